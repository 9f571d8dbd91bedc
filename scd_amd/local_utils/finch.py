"""Drop-in for the reference's local_utils/finch.py (FINCH :106-173) on libscd_hip.so: same name, arguments and return types; cosine
distance only (docs/design/finch.md)."""
from ..finch import FINCH, Finch  # noqa: F401
