"""Tensor-level wrappers over the C ABI (include/scd_hip.h).

torch is plumbing here: it owns device memory and the current stream; every
computation below is a call into libscd_hip.so.  Nothing in this module falls
back to torch math - a missing library or device raises.
"""
import ctypes as C
import os

import numpy as np
import weakref

import torch

from . import _lib
from ._lib import check, ptr, SCD_F16, SCD_F32, SIM_RAW, SIM_SOFTMAX

_L = _lib.load
_dev = [None]           # device of the tensors of the op being issued: the handle and the stream follow the DATA, not torch's current device


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.ScdError(_lib.SCD_EINVAL, "tensor must live on the HIP device (got %s)" % t.device)
    for t in ts:
        if t is not None:
            _dev[0] = t.device.index
            break


def handle():
    return _lib.handle(_dev[0])


def stream_ptr():
    if _dev[0] is not None and _dev[0] != torch.cuda.current_device():
        raise _lib.ScdError(_lib.SCD_EINVAL, "tensors live on cuda:%d but the current device is cuda:%d (use torch.cuda.device / "
                            "set_device: kernels are launched on the current device's stream)" % (_dev[0], torch.cuda.current_device()))
    return _lib.stream_ptr()


def _ws(nbytes, device):
    return torch.empty(int(nbytes), dtype=torch.uint8, device=device)


def trace_mark(end=False):
    """An empty marker kernel on the current stream (scd_mark_begin_kernel / scd_mark_end_kernel): brackets a measured region in a
    rocprofv3 kernel trace."""
    check(_L().scd_trace_mark(handle(), 1 if end else 0, stream_ptr()))


# ----------------------------------------------------------------------------- normalise / layout
def l2norm_rows(x):
    """F.normalize(x, dim=-1) (main_unsup.py:130)."""
    _need_cuda(x)
    x = x.contiguous()
    out = torch.empty_like(x)
    dt = {torch.float32: SCD_F32, torch.float16: SCD_F16}[x.dtype]
    check(_L().scd_l2norm_rows(handle(), ptr(x), dt, x.shape[0], x.shape[1], ptr(out), stream_ptr()))
    return out


def transpose_f16(w):
    """[r,c] fp16 -> [c,r] (zeroshot_weights [512,V] -> name-major Wt [V,512])."""
    _need_cuda(w)
    w = w.contiguous()
    out = torch.empty((w.shape[1], w.shape[0]), dtype=torch.float16, device=w.device)
    check(_L().scd_transpose_f16(handle(), ptr(w), w.shape[0], w.shape[1], ptr(out), stream_ptr()))
    return out


def gather_rows_f16(wt, idx):
    _need_cuda(wt, idx)
    idx = idx.to(torch.int64).contiguous()
    out = torch.empty((idx.numel(), wt.shape[1]), dtype=torch.float16, device=wt.device)
    check(_L().scd_gather_rows_f16(handle(), ptr(wt), ptr(idx), idx.numel(), wt.shape[1], ptr(out), stream_ptr()))
    return out


def select_rows(feats16, idx, name_idx=None, want16=True, want32=True):
    """`all_feats[mask]` (main_unsup.py:318-321) for the rows `idx` (device int64) of the fp16 feature matrix, in one launch: returns
    (rows fp16 or None, rows float32 or None, name_idx[idx] or None)."""
    _need_cuda(feats16, idx)
    assert feats16.dtype == torch.float16 and feats16.is_contiguous() and idx.dtype == torch.int64
    m, d = idx.numel(), feats16.shape[1]
    dev = feats16.device
    o16 = torch.empty((m, d), dtype=torch.float16, device=dev) if want16 else None
    o32 = torch.empty((m, d), dtype=torch.float32, device=dev) if want32 else None
    k = 0
    on = None
    if name_idx is not None:
        assert name_idx.dtype == torch.int64 and name_idx.is_contiguous()
        k = name_idx.shape[1]
        on = torch.empty((m, k), dtype=torch.int64, device=dev)
    if m:
        check(_L().scd_select_rows(handle(), ptr(feats16), ptr(name_idx), ptr(idx), m, d, k, ptr(o16), ptr(o32), ptr(on), stream_ptr()))
    return o16, o32, on


def mean2_f16(a, b):
    """fp16((a + b) / 2): the textual-enhancement feature (main_unsup.py:518 commented formula)."""
    _need_cuda(a, b)
    a, b = a.to(torch.float16).contiguous(), b.to(torch.float16).contiguous()
    assert a.shape == b.shape
    out = torch.empty_like(a)
    check(_L().scd_mean2_f16(handle(), ptr(a), ptr(b), a.numel(), ptr(out), stream_ptr()))
    return out


# ----------------------------------------------------------------------------- similarity
_frozen_vocabs = {}      # id(wt) -> (weakref, data_ptr, _version, shape, norm tensor, stream pointer, event): ops.freeze_vocab


def _vocab_norm_now(wt):
    out = torch.empty(1, dtype=torch.int32, device=wt.device)
    check(_L().scd_sim_vocab_norm(handle(), ptr(wt), wt.shape[0], wt.shape[1], ptr(out), stream_ptr()))
    return out


def freeze_vocab(wt):
    """The caller's promise that the name-major fp16 vocabulary `wt` will not be written any more (by anybody: torch, a kernel of this
    library writing through the raw pointer, another stream): its max ||w||^2 - the data-dependent part of the similarity filter's
    error bound - is computed once, here, and every later sim_topk on the tensor reuses it.  Without the promise the norm is computed
    per call (12 us beside a 2.7-ms call at C2): torch's `_version` does not see raw-pointer writes, and a stale, too small norm would
    certify rows it must not.  `unfreeze_vocab` takes the promise back.  Returns wt."""
    _need_cuda(wt)
    assert wt.dtype == torch.float16 and wt.is_contiguous() and wt.dim() == 2
    ev = torch.cuda.Event()
    norm = _vocab_norm_now(wt)
    ev.record()
    if len(_frozen_vocabs) > 64:
        for kk in [kk for kk, e in _frozen_vocabs.items() if e[0]() is None]:
            del _frozen_vocabs[kk]
    _frozen_vocabs[id(wt)] = (weakref.ref(wt), wt.data_ptr(), wt._version, tuple(wt.shape), norm, torch.cuda.current_stream().cuda_stream, ev)
    return wt


def unfreeze_vocab(wt):
    _frozen_vocabs.pop(id(wt), None)


def vocab_norm(wt):
    """max_v ||w_v||^2 of a name-major fp16 vocabulary (scd_sim_vocab_norm): the frozen tensor's stored value (ops.freeze_vocab; a
    consumer on another stream first waits for the event recorded behind its computation), a fresh one otherwise.  An in-place torch
    write after the freeze (`_version`) ends the promise as well."""
    ent = _frozen_vocabs.get(id(wt))
    if ent is not None and ent[0]() is wt and ent[1] == wt.data_ptr() and ent[2] == wt._version and ent[3] == tuple(wt.shape):
        if ent[5] != torch.cuda.current_stream().cuda_stream:
            ent[6].wait()                     # the current stream waits for the norm's kernel
        return ent[4]
    if ent is not None:
        del _frozen_vocabs[id(wt)]
    return _vocab_norm_now(wt)


def sim_topk(f, wt, k, mode="raw", scale=100.0, return_fallback=False):
    """Top-k of scale * f @ wt.T per row.  f [n,d] fp16, wt [v,d] fp16 (name-major).
    Returns (idx int64 [n,k], val float32 [n,k])."""
    _need_cuda(f, wt)
    f = f.to(torch.float16).contiguous()
    wt_in = wt
    wt = wt.to(torch.float16).contiguous()
    n, d = f.shape
    v = wt.shape[0]
    idx = torch.empty((n, k), dtype=torch.int64, device=f.device)
    val = torch.empty((n, k), dtype=torch.float32, device=f.device)
    fb = torch.empty(1, dtype=torch.int32, device=f.device) if return_fallback else None      # written by the library when asked for
    nb = _L().scd_sim_topk_ws_bytes(n, d, v, k)
    ws = _ws(nb, f.device)
    m = SIM_SOFTMAX if mode == "softmax" else SIM_RAW
    if wt is wt_in and id(wt) in _frozen_vocabs:
        # a vocabulary the caller froze (ops.freeze_vocab: the full vocabulary of main_unsup.py:504-531, reused by every call): its norm once
        check(_L().scd_sim_topk_prenorm(handle(), ptr(f), ptr(wt), n, d, v, float(scale), k, m, ptr(idx), ptr(val), ptr(fb),
                                        ptr(ws), nb, ptr(vocab_norm(wt)), stream_ptr()))
    else:
        check(_L().scd_sim_topk(handle(), ptr(f), ptr(wt), n, d, v, float(scale), k, m, ptr(idx), ptr(val), ptr(fb),
                                ptr(ws), nb, stream_ptr()))
    if return_fallback:
        return idx, val, fb
    return idx, val


def sim_argmax(f, wsel_t, scale=100.0):
    """argmax(scale * f @ wsel_t.T, -1) (main_unsup.py:603-614): scd_sim_argmax.  Returns (idx int64 [n], val float32 [n])."""
    _need_cuda(f, wsel_t)
    f = f.to(torch.float16).contiguous()
    wt = wsel_t.to(torch.float16).contiguous()
    n, d = f.shape
    v = wt.shape[0]
    idx = torch.empty(n, dtype=torch.int64, device=f.device)
    val = torch.empty(n, dtype=torch.float32, device=f.device)
    nb = _L().scd_sim_topk_ws_bytes(n, d, v, 1)
    ws = _ws(nb, f.device)
    check(_L().scd_sim_argmax(handle(), ptr(f), ptr(wt), n, d, v, float(scale), ptr(idx), ptr(val), ptr(ws), nb, stream_ptr()))
    return idx, val


SIM_PATH_RB8, SIM_PATH_RC16, SIM_PATH_TILE, SIM_PATH_TILE768, SIM_PATH_SPLIT, SIM_PATH_REFINE4 = 1, 2, 4, 8, 16, 32     # include/scd_hip.h


def sim_last_path():
    """The kernels the last sim_topk / sim_argmax call of this process launched (scd_sim_last_path: a set of SIM_PATH_* bits)."""
    return _L().scd_sim_last_path()


def prompt_pool(emb, n_names, t_per, out, col0):
    """normalise -> mean -> normalise of each name's prompt embeddings into columns of out [d, V]."""
    _need_cuda(emb, out)
    check(_L().scd_prompt_pool(handle(), ptr(emb), n_names, t_per, emb.shape[1], col0, out.shape[1], ptr(out), stream_ptr()))


# ----------------------------------------------------------------------------- k-means
def kmeans_timing(enable, cap=4096):
    """HIP-event timing of the streaming E-step kernel inside scd_kmeans_estep / scd_kmeans_lloyd_step (measurement aid).
    Returns the durations (ms, numpy, call order) collected since the last call and switches the collection on / off."""
    buf = np.zeros(cap, dtype=np.float64)
    cnt = C.c_int(0)
    check(_L().scd_kmeans_timing(handle(), 1 if enable else 0, ptr(buf), cap, C.byref(cnt)))
    return buf[: min(cnt.value, cap)].copy()


ESTEP_FEW, ESTEP_CENTRES_FROM_FINALIZE, LLOYD_FULL = 1, 2, 8      # include/scd_hip.h
_LAST_FINALIZE = {}                                  # "c": (weakref to the centres kmeans_finalize returned, their _version, the KMeansData)


class KMeansData:
    """X (float32 [n,d], device) plus the prepared fp16 E-step operand."""

    def __init__(self, x):
        _need_cuda(x)
        self.x = x.to(torch.float32).contiguous()
        self.n, self.d = self.x.shape
        self.prep = _ws(_L().scd_kmeans_prep_bytes(self.n, self.d), self.x.device)
        check(_L().scd_kmeans_prepare(handle(), ptr(self.x), self.n, self.d, ptr(self.prep), stream_ptr()))
        self._ws = {}

    def ws(self, key, nbytes):
        w = self._ws.get(key)
        if w is None or w.numel() < nbytes:
            w = self._ws[key] = _ws(nbytes, self.x.device)
        return w

    def estep(self, centers, return_refined=False, expect_few=False):
        """expect_few: few rows are expected inside the filter's error bound (late Lloyd iterations): they are re-evaluated in
        the filter kernel's tail, no refine launch.  Same labels either way."""
        _need_cuda(self.x)
        k = centers.shape[0]
        # the hand-over of kmeans_finalize(data=self) is used only for the very tensor it returned, unmodified since (torch counts
        # in-place writes in `_version`): a matching address alone proves nothing, the allocator recycles addresses
        last = _LAST_FINALIZE.get("c")
        vouch = last is not None and last[0]() is centers and last[1] == centers._version and last[2] is self
        _LAST_FINALIZE.pop("c", None)
        flags = (ESTEP_FEW if expect_few else 0) | (ESTEP_CENTRES_FROM_FINALIZE if vouch else 0)
        check(_L().scd_kmeans_estep_hint(handle(), flags))
        centers = centers.to(torch.float32).contiguous()
        labels = torch.empty(self.n, dtype=torch.int32, device=self.x.device)
        ref = torch.zeros(1, dtype=torch.int32, device=self.x.device) if return_refined else None     # (a fill launch otherwise)
        nb = _L().scd_kmeans_estep_ws_bytes(self.n, self.d, k)
        ws = self.ws(("e", k), nb)
        check(_L().scd_kmeans_estep(handle(), ptr(self.x), ptr(self.prep), ptr(centers), self.n, self.d, k, ptr(labels),
                                    ptr(ref), ptr(ws), nb, stream_ptr()))
        return (labels, ref) if return_refined else labels

    def rowdist(self, centers, labels):
        _need_cuda(self.x)
        centers = centers.to(torch.float32).contiguous()
        out = torch.empty(self.n, dtype=torch.float32, device=self.x.device)
        check(_L().scd_kmeans_rowdist(handle(), ptr(self.x), ptr(centers), ptr(labels), self.n, self.d, centers.shape[0],
                                      ptr(out), stream_ptr()))
        return out

    def min_update(self, c_new, d2):
        _need_cuda(self.x)
        c_new = c_new.to(torch.float32).contiguous()
        check(_L().scd_kmeans_min_update(handle(), ptr(self.x), ptr(c_new), self.n, self.d, ptr(d2), stream_ptr()))

    def dist(self, centers, sqrt=False, with_cost=False):
        _need_cuda(self.x)
        centers = centers.to(torch.float32).contiguous()
        k = centers.shape[0]
        out = torch.empty((self.n, k), dtype=torch.float32, device=self.x.device)
        cost = torch.empty((self.n, k), dtype=torch.int32, device=self.x.device) if with_cost else None
        check(_L().scd_kmeans_dist(handle(), ptr(self.x), ptr(centers), self.n, self.d, k, 1 if sqrt else 0, ptr(out), ptr(cost),
                                   stream_ptr()))
        return (out, cost) if with_cost else out


def f16_exact(x):
    """fp16 copy of x if every value survives the round trip (features that left an fp16 encoder), else None.  One device
    read-back per data set; the copy halves the bytes the M-step streams per Lloyd iteration."""
    _need_cuda(x)
    x = x.to(torch.float32).contiguous()
    if x.numel() % 4 or x.shape[-1] % 2:
        return None
    out = torch.empty(x.shape, dtype=torch.float16, device=x.device)
    res = torch.empty(2, dtype=torch.int32, device=x.device)                  # [inexact blocks | max |x| as float bits]
    check(_L().scd_f16_exact_max(handle(), ptr(x), x.numel(), ptr(out), ptr(res), res.data_ptr() + 4, stream_ptr()))
    host = res.cpu()
    if int(host[0]) != 0:
        return None
    # max |x| rides along on the copy: the incremental M-step's exact-sums argument needs rows * max|x| < 2^29 as well
    # (LloydBuffers.inc); a plain attribute of the tensor object, not of its storage
    out.scd_absmax = float(host[1:].view(torch.float32)[0])
    return out


def kmeans_mstep(x, labels32, c_old, k, split=0, x16=None):
    """(sums float64 [k,d], counts int64 [k], inertia float64 [2]) partials of one rank.  x16: the exact fp16 copy of x
    (f16_exact), streamed instead of x."""
    _need_cuda(x, labels32)
    n, d = x.shape
    sums = torch.empty((k, d), dtype=torch.float64, device=x.device)
    counts = torch.empty(k, dtype=torch.int64, device=x.device)
    inertia = torch.empty(2, dtype=torch.float64, device=x.device)          # zeroed by the library (no torch fill launch)
    nb = _L().scd_kmeans_mstep_ws_bytes(n, d, k)
    ws = _ws(nb, x.device)
    if x16 is not None:
        check(_L().scd_kmeans_mstep_f16(handle(), ptr(x16), ptr(labels32), ptr(c_old), n, d, k, int(split), ptr(sums), ptr(counts),
                                        ptr(inertia), ptr(ws), nb, stream_ptr()))
    else:
        check(_L().scd_kmeans_mstep(handle(), ptr(x), ptr(labels32), ptr(c_old), n, d, k, int(split), ptr(sums), ptr(counts),
                                    ptr(inertia), ptr(ws), nb, stream_ptr()))
    return sums, counts, inertia


def _dd_add(a, b):
    """(hi, lo) + (hi, lo) in double-double (Knuth's two-sum on the high parts); host floats."""
    s_ = a[0] + b[0]
    bb = s_ - a[0]
    e = (a[0] - (s_ - bb)) + (b[0] - bb)
    e += a[1] + b[1]
    hi = s_ + e
    return hi, e - (hi - s_)


class LloydBuffers:
    """Device buffers of KMeansEngine's Lloyd loop through scd_kmeans_lloyd_step[_delta]: two sets (the host reads set i while the
    device fills set i + 1), allocated once per fit.  With an exact fp16 copy of the rows (`cat16`) the M-step can run
    incrementally (`step_delta`: sums / counts updated with the rows whose label changed, inertia from the sums)."""

    def __init__(self, data_u, cat, cat16, k, dd=None):
        """dd: the process group's exchange object (scd_amd.kmeans._Dist: allreduce_(t, op), allgather(t)) when `cat` is one rank's row
        shard - only `run` is shard-aware (scd_kmeans_lloyd_run_sharded), and only when EVERY rank's rows qualify (self.inc)."""
        dev = cat.device
        n_cat, d = cat.shape
        self.data, self.cat, self.cat16, self.k, self.dd = data_u, cat, cat16, k, dd
        self.lab32 = torch.empty(n_cat, dtype=torch.int32, device=dev)
        self.c = [torch.empty((k, d), dtype=torch.float32, device=dev) for _ in range(2)]
        # a run's initial centres get a buffer of their own: the hand-over of scd_kmeans_finalize is keyed on the centre POINTER, and
        # one of self.c may still be registered (with the previous run's last centres) when the next restart begins
        self.c0 = torch.empty((k, d), dtype=torch.float32, device=dev)
        self.sums = torch.empty((k, d), dtype=torch.float64, device=dev)
        self.counts = torch.empty(k, dtype=torch.int64, device=dev)
        # {inertia labelled, inertia unlabelled, centre shift, rows re-evaluated exactly, rows whose label changed}
        self.stats = [torch.zeros(5, dtype=torch.float64, device=dev) for _ in range(2)]
        # incremental exact M-step: every float64 cluster sum must be exact, i.e. rows * max|x| * 2^24 < 2^53 on top of the exact fp16
        # copy (unit-scale features: 1e5 * 1 against 5e8; fp16 values near 65504 in big clusters, or infinities, take the fresh M-step)
        amax = getattr(cat16, "scd_absmax", float("inf")) if cat16 is not None else float("inf")
        n_glob = n_cat
        if dd is not None:
            # the bound is on the GLOBAL cluster sums, and all ranks must take the same path (its collectives differ from the other's):
            # [rows] summed, [max|x|, "my rows do not qualify"] maximised
            tot = dd.allreduce_(torch.tensor([float(n_cat)], dtype=torch.float64, device=dev))
            bad = cat16 is None or not np.isfinite(amax) or data_u.n <= 0
            mx = dd.allreduce_(torch.tensor([0.0 if bad else float(amax), 1.0 if bad else 0.0], dtype=torch.float64, device=dev), op="max")
            tot_h, mx_h = tot.cpu().numpy(), mx.cpu().numpy()
            n_glob, amax = float(tot_h[0]), (float("inf") if mx_h[1] > 0 else float(mx_h[0]))
        # (rank-local sizing only after the ranks have agreed above: KMeansEngine.fit has also agreed that no shard is empty)
        self.nb_e = _L().scd_kmeans_estep_ws_bytes(data_u.n, data_u.d, k)
        self.ws_e = data_u.ws(("e", k), self.nb_e)
        self.nb_m = _L().scd_kmeans_mstep_ws_bytes(n_cat, d, k)
        self.ws_m = _ws(self.nb_m, dev)
        self.inc = (cat16 is not None and k <= 8192 and n_glob * amax < 2.0 ** 29 and os.environ.get("SCD_MSTEP_DELTA", "1") != "0")
        if self.inc:
            if dd is not None:
                self.xbuf = torch.empty(k * d + 2 * k, dtype=torch.float64, device=dev)     # [sums | counts as float64 | int64 counts]
                self._xch_err = None
                view = self.xbuf[: k * d + k]

                def _cb(ctx, buf, n_doubles, stream):
                    # called by scd_kmeans_lloyd_run_sharded between an iteration's M-step and its finalize launch, on the stream the
                    # kernels are enqueued on (torch's current stream, which is what dist.all_reduce orders itself against)
                    try:
                        dd.allreduce_(view)
                        return 0
                    except BaseException as e:          # never let an exception unwind through the C frames
                        self._xch_err = e
                        return 1
                self._xch_cb = _lib.EXCHANGE_FN(_cb)
            self.lab_prev = torch.full((n_cat,), -1, dtype=torch.int32, device=dev)
            self.sumsq = torch.empty(4, dtype=torch.float64, device=dev)
            self.sums_lab = self.counts_lab = None
            self._fit_ready = False
            # scd_kmeans_lloyd_run: iteration i's labels / centres in slot i % 3 of these rings
            self.c_ring = torch.empty((3, k, d), dtype=torch.float32, device=dev)
            self.stats_ring = torch.zeros((2, 5), dtype=torch.float64, device=dev)
            self.lab_ring = torch.empty((3, n_cat), dtype=torch.int32, device=dev)
            self.result = np.zeros(4, dtype=np.float64)

    def step(self, c_in, c_out, stats, expect_few):
        d = self.data
        # the hand-over is vouched for only when c_in is the buffer the previous step of THIS object wrote (private buffers, nothing
        # else writes them); c0 is a fresh seeding no finalize produced, and its address may be a recycled one
        flags = (ESTEP_FEW if expect_few else 0) | (ESTEP_CENTRES_FROM_FINALIZE if c_in is not self.c0 else 0)
        check(_L().scd_kmeans_lloyd_step(handle(), ptr(d.x), ptr(d.prep), d.n, ptr(self.cat), ptr(self.cat16), self.cat.shape[0],
                                         d.d, self.k, ptr(self.lab32), ptr(c_in), ptr(c_out), ptr(self.sums), ptr(self.counts),
                                         ptr(stats), flags, ptr(self.ws_e), self.nb_e, ptr(self.ws_m), self.nb_m,
                                         stream_ptr()))

    def _prepare_fit(self):
        """Once per fit: the rows' sums of squares (labelled | unlabelled, double-double) and the sums / counts of the labelled rows,
        whose labels (self.lab32[:l_num], set by the caller) never change."""
        n_cat, d = self.cat.shape
        l_num = n_cat - self.data.n
        check(_L().scd_kmeans_sumsq(handle(), ptr(self.cat16), None, n_cat, d, l_num, ptr(self.sumsq), stream_ptr()))
        dd = self.dd
        any_lab = l_num > 0
        if dd is not None:
            # global sums of squares: the ranks' double-double pairs added in rank order on the host (once per fit); global sums /
            # counts of the labelled rows (exact sums: any order)
            parts = dd.allgather(self.sumsq).cpu().numpy()
            acc = [(0.0, 0.0), (0.0, 0.0)]
            for r in range(parts.shape[0]):
                acc = [_dd_add(acc[0], (float(parts[r, 0]), float(parts[r, 1]))), _dd_add(acc[1], (float(parts[r, 2]), float(parts[r, 3])))]
            self.sumsq.copy_(torch.tensor([acc[0][0], acc[0][1], acc[1][0], acc[1][1]], dtype=torch.float64))
            any_lab = bool(dd.allreduce_(torch.tensor([float(l_num)], dtype=torch.float64, device=self.cat.device)).item() > 0)
        if any_lab:
            if l_num > 0:
                s, c, _ = kmeans_mstep(self.cat[:l_num], self.lab32[:l_num].contiguous(), None, self.k, 0, x16=self.cat16[:l_num])
            else:
                s = torch.zeros((self.k, d), dtype=torch.float64, device=self.cat.device)
                c = torch.zeros(self.k, dtype=torch.int64, device=self.cat.device)
            if dd is not None:
                dd.allreduce_(s)
                dd.allreduce_(c)
            self.sums_lab, self.counts_lab = s.contiguous(), c.contiguous()
        self._fit_ready = True

    def step_delta(self, c_in, c_out, stats, expect_few, full):
        """One Lloyd iteration with the incremental M-step (full=False) or with a fresh one that also re-bases the incremental
        state (full=True: the first iterations of a restart, or when many labels are moving)."""
        if not self._fit_ready:
            self._prepare_fit()
        d = self.data
        flags = (ESTEP_FEW if expect_few else 0) | (ESTEP_CENTRES_FROM_FINALIZE if c_in is not self.c0 else 0) | (LLOYD_FULL if full else 0)
        check(_L().scd_kmeans_lloyd_step_delta(handle(), ptr(d.x), ptr(d.prep), d.n, ptr(self.cat16), self.cat.shape[0], d.d, self.k,
                                               ptr(self.lab32), ptr(self.lab_prev), ptr(c_in), ptr(c_out), ptr(self.sums), ptr(self.counts),
                                               ptr(self.sums_lab), ptr(self.counts_lab), ptr(self.sumsq), ptr(stats), flags,
                                               ptr(self.ws_e), self.nb_e, ptr(self.ws_m), self.nb_m, stream_ptr()))


    def run(self, max_iter, tol):
        """A whole restart from self.c0 (the seeding; labelled rows' labels in self.lab32[:l_num]) behind one call:
        scd_kmeans_lloyd_run.  Returns (labels int32 [n_cat], float32 inertia, centres [k, d], iterations done, iterations with the
        incremental M-step, iterations launched) of the least-inertia iteration - fresh tensors."""
        if not self._fit_ready:
            self._prepare_fit()
        d = self.data
        n_cat = self.cat.shape[0]
        best_lab = torch.empty(n_cat, dtype=torch.int32, device=self.cat.device)
        best_c = torch.empty((self.k, d.d), dtype=torch.float32, device=self.cat.device)
        args = (handle(), ptr(d.x), ptr(d.prep), d.n, ptr(self.cat16), n_cat, d.d, self.k,
                ptr(self.lab32) if n_cat > d.n else None, ptr(self.lab_ring), ptr(self.lab_prev), ptr(self.c0),
                ptr(self.c_ring), ptr(self.sums), ptr(self.counts), ptr(self.sums_lab), ptr(self.counts_lab),
                ptr(self.sumsq), ptr(self.stats_ring), int(max_iter), float(tol), ptr(best_lab), ptr(best_c),
                self.result.ctypes.data, ptr(self.ws_e), self.nb_e, ptr(self.ws_m), self.nb_m, stream_ptr())
        if self.dd is None:
            check(_L().scd_kmeans_lloyd_run(*args))
        else:
            # a row shard: every iteration's [sums | counts] go through the group's all-reduce (the callback) before the centres are formed
            self._xch_err = None
            rc = _L().scd_kmeans_lloyd_run_sharded(*args, ptr(self.xbuf), self._xch_cb, None)
            if self._xch_err is not None:
                raise self._xch_err
            check(rc)
        r = self.result
        return best_lab, np.float32(r[0]), best_c, int(r[1]), int(r[2]), int(r[3])


    def run_multi(self, c_inits, max_iter, tol, n_streams=0):
        """ALL restarts of the fit in lock-step behind one call (scd_kmeans_lloyd_run_multi): c_inits float32 [R, k, d] are the restarts'
        seedings (labelled rows' labels in self.lab32[:l_num], shared).  Under a process group ONE all-reduce per iteration carries every
        running restart's [sums | counts].  Returns a list of run()'s tuples, restart by restart - the same bits as R calls of run()."""
        if not self._fit_ready:
            self._prepare_fit()
        d = self.data
        dev = self.cat.device
        n_cat, k, dim = self.cat.shape[0], self.k, d.d
        R = int(c_inits.shape[0])
        c_inits = c_inits.to(torch.float32).contiguous()
        hs = _lib.extra_handles(R)
        per = getattr(self, "_multi", None)
        if per is None or per["R"] != R:
            per = self._multi = dict(
                R=R, lab_ring=torch.empty((R, 3, n_cat), dtype=torch.int32, device=dev), lab_prev=torch.full((R, n_cat), -1, dtype=torch.int32, device=dev),
                c_ring=torch.empty((R, 3, k, dim), dtype=torch.float32, device=dev), sums=torch.empty((R, k, dim), dtype=torch.float64, device=dev),
                counts=torch.empty((R, k), dtype=torch.int64, device=dev), stats_ring=torch.zeros((R, 2, 5), dtype=torch.float64, device=dev),
                ws_m=[_ws(self.nb_m, dev) for _ in range(R)],
                result=np.zeros((R, 4), dtype=np.float64))
            # the restarts' E-step workspaces as equal strides of ONE buffer: one allocation per fit instead of R
            stride = (int(self.nb_e) + 255) // 256 * 256
            per["ws_e_all"] = _ws(R * stride, dev)
            per["ws_e"] = [per["ws_e_all"][j * stride:(j + 1) * stride] for j in range(R)]
            if self.dd is not None:
                xb = per["xbuf"] = torch.empty(R * (k * dim + 2 * k), dtype=torch.float64, device=dev)
                dd = self.dd

                def _cb(ctx, buf, n_doubles, stream):
                    try:
                        dd.allreduce_(xb[: int(n_doubles)])          # the running restarts' [sums | counts], densely packed
                        self._xch_n = getattr(self, "_xch_n", 0) + 1
                        return 0
                    except BaseException as e:          # never let an exception unwind through the C frames
                        self._xch_err = e
                        return 1
                per["cb"] = _lib.EXCHANGE_FN(_cb)
        best_lab = torch.empty((R, n_cat), dtype=torch.int32, device=dev)
        best_c = torch.empty((R, k, dim), dtype=torch.float32, device=dev)
        arr = (_lib.LloydRestart * R)()
        for j in range(R):
            a = arr[j]
            a.h = hs[j].value
            a.lab_ring, a.labels_prev = per["lab_ring"][j].data_ptr(), per["lab_prev"][j].data_ptr()
            a.C_start, a.C_ring = c_inits[j].data_ptr(), per["c_ring"][j].data_ptr()
            a.sums, a.counts, a.stats_ring = per["sums"][j].data_ptr(), per["counts"][j].data_ptr(), per["stats_ring"][j].data_ptr()
            a.best_labels, a.best_C = best_lab[j].data_ptr(), best_c[j].data_ptr()
            a.result_host = per["result"][j].ctypes.data
            a.ws_e, a.ws_m = per["ws_e"][j].data_ptr(), per["ws_m"][j].data_ptr()
        self._xch_err = None
        rc = _L().scd_kmeans_lloyd_run_multi(C.cast(arr, C.c_void_p), R, ptr(d.x), ptr(d.prep), d.n, ptr(self.cat16), n_cat, dim, k,
                                             ptr(self.lab32) if n_cat > d.n else None, ptr(self.sums_lab), ptr(self.counts_lab), ptr(self.sumsq),
                                             int(max_iter), float(tol), self.nb_e, self.nb_m, stream_ptr(),
                                             ptr(per["xbuf"]) if self.dd is not None else None,
                                             C.cast(per["cb"], C.c_void_p) if self.dd is not None else None, None, int(n_streams))
        if self._xch_err is not None:
            raise self._xch_err
        check(rc)
        res = per["result"]
        return [(best_lab[j], np.float32(res[j, 0]), best_c[j], int(res[j, 1]), int(res[j, 2]), int(res[j, 3])) for j in range(R)]

    def run_sk(self, max_iter, tol):
        """sklearn's `_kmeans_single_lloyd` from self.c0 behind one call (scd_kmeans_lloyd_run_sk; no labelled rows).  Returns
        (labels int32 [n], centres [k, d], n_iter) - the E-step of the final centres and those centres, fresh tensors - or None when an
        iteration left a cluster empty (sklearn relocates it; the caller runs that start through its own loop)."""
        if not self._fit_ready:
            self._prepare_fit()
        d = self.data
        n = self.cat.shape[0]
        assert n == d.n and self.inc
        self.lab_prev.fill_(-1)
        lab = torch.empty(n, dtype=torch.int32, device=self.cat.device)
        cen = torch.empty((self.k, d.d), dtype=torch.float32, device=self.cat.device)
        check(_L().scd_kmeans_lloyd_run_sk(handle(), ptr(d.x), ptr(d.prep), d.n, ptr(self.cat16), d.d, self.k, ptr(self.lab_ring),
                                           ptr(self.lab_prev), ptr(self.c0), ptr(self.c_ring), ptr(self.sums), ptr(self.counts),
                                           ptr(self.sumsq), ptr(self.stats_ring), int(max_iter), float(tol), ptr(lab), ptr(cen),
                                           self.result.ctypes.data, ptr(self.ws_e), self.nb_e, ptr(self.ws_m), self.nb_m, stream_ptr()))
        r = self.result
        if r[0] != 0:
            return None
        return lab, cen, int(r[1])


def kpp_greedy_lockstep(x, x16, first, u, k):
    """scikit-learn's greedy k-means++ for R starts in lock-step (scd_kpp_greedy_lockstep).  x float32 [n, d]; x16 its exact fp16 copy
    or None; first: host int64 [R] (the starts' first centres); u: host float64 [R, k - 1, L] (the uniforms each start's RandomState
    slice provides, L per added centre).  Returns (centres float32 [R, k, d], picks int64 [k, R]) on the device."""
    _need_cuda(x)
    n, d = x.shape
    first = np.ascontiguousarray(first, dtype=np.int64)
    r = first.shape[0]
    u = np.ascontiguousarray(u, dtype=np.float64).reshape(r, max(k - 1, 0), -1)
    ell = u.shape[2] if k > 1 else 1
    dev = x.device
    first_d = torch.from_numpy(first).to(dev)
    u_d = torch.from_numpy(np.ascontiguousarray(u.transpose(1, 0, 2))).to(dev) if k > 1 else None       # [k - 1][R][L]
    cbuf = torch.empty((r, k, d), dtype=torch.float32, device=dev)
    picks = torch.empty((k, r), dtype=torch.int64, device=dev)
    nb = _L().scd_kpp_greedy_ws_bytes(n, d, r, ell)
    ws = _ws(nb, dev)
    check(_L().scd_kpp_greedy_lockstep(handle(), ptr(x), ptr(x16), n, d, r, ell, k, ptr(first_d), ptr(u_d), ptr(cbuf), ptr(picks),
                                       ptr(ws), nb, stream_ptr()))
    return cbuf, picks


def kmeans_finalize(sums, counts, c_old=None, shift_mode=0, data=None):
    """shift_mode 0: (sum_k ||dc_k||)^2 (the reference's SSKM test); 1: sum_k ||dc_k||^2 (sklearn's center_shift_tot).
    data (a KMeansData): the centres' E-step operands are produced by the same launch, for the next data.estep(centres)."""
    _need_cuda(sums)
    k, d = sums.shape
    c = torch.empty((k, d), dtype=torch.float32, device=sums.device)
    shift = torch.empty(1, dtype=torch.float64, device=sums.device)
    prep, ws, nb, n = None, None, 0, 0
    if data is not None and data.d == d:
        nb = _L().scd_kmeans_estep_ws_bytes(data.n, d, k)
        prep, ws, n = data.prep, data.ws(("e", k), nb), data.n
    check(_L().scd_kmeans_finalize(handle(), ptr(sums), ptr(counts), k, d, ptr(c_old), ptr(c), ptr(shift), int(shift_mode),
                                   ptr(prep), ptr(ws), nb, n, stream_ptr()))
    if data is not None and data.d == d:
        _LAST_FINALIZE["c"] = (weakref.ref(c), c._version, data)
    else:
        _LAST_FINALIZE.pop("c", None)
    return c, shift


def labels_changed(a, b):
    """Number of rows where two int32 label vectors differ (device int64[1])."""
    _need_cuda(a, b)
    out = torch.empty(1, dtype=torch.int64, device=a.device)
    check(_L().scd_labels_changed(handle(), ptr(a), ptr(b), a.numel(), ptr(out), stream_ptr()))
    return out


def kpp_searchsorted(d2, u):
    """sklearn's k-means++ candidate draw: searchsorted(cumsum_f64(d2), u * float32(sum d2)) for every uniform in u (host
    floats).  Returns (idx int64 [L] on the device, pot float64[1])."""
    _need_cuda(d2)
    uu = torch.as_tensor(np.asarray(u, dtype=np.float64)).to(d2.device)
    idx = torch.empty(uu.numel(), dtype=torch.int64, device=d2.device)
    pot = torch.empty(1, dtype=torch.float64, device=d2.device)
    nb = _L().scd_kpp_draw_ws_bytes(d2.numel())
    ws = _kpp_ws.get((d2.device, nb))
    if ws is None:
        ws = _kpp_ws[(d2.device, nb)] = _ws(nb, d2.device)
    check(_L().scd_kpp_searchsorted(handle(), ptr(d2), d2.numel(), ptr(uu), uu.numel(), ptr(idx), ptr(pot), ptr(ws), nb, stream_ptr()))
    return idx, pot


def kpp_draw(d2, r, total=None, prefix=None, want_idx=True, want_probsum=False):
    """Device-side k-means++ draw.  Returns (idx int64[1] or None, probsum float64[1] or None); idx -1 = no hit."""
    _need_cuda(d2)
    idx = torch.empty(1, dtype=torch.int64, device=d2.device) if want_idx else None
    ps = torch.empty(1, dtype=torch.float64, device=d2.device) if want_probsum else None
    nb = _L().scd_kpp_draw_ws_bytes(d2.numel())
    ws = _kpp_ws.get((d2.device, nb))
    if ws is None:
        ws = _kpp_ws[(d2.device, nb)] = _ws(nb, d2.device)
    check(_L().scd_kpp_draw(handle(), ptr(d2), d2.numel(), float(np.float32(r)), ptr(total), ptr(prefix), ptr(idx), ptr(ps),
                            ptr(ws), nb, stream_ptr()))
    return idx, ps


_kpp_ws = {}


def min_update_multi(x, c_new, d2):
    """d2[r] = min(d2[r], ||x - c_new[r]||^2) for the R rows of c_new at once (x read once).  d2 float32 [R, n], in place."""
    _need_cuda(x, c_new, d2)
    c_new = c_new.to(torch.float32).contiguous()
    n, d = x.shape
    check(_L().scd_kmeans_min_update_multi(handle(), ptr(x), ptr(c_new), n, d, c_new.shape[0], ptr(d2), d2.stride(0), stream_ptr()))


def kpp_draw_multi(d2, r, total=None, prefix=None, want_idx=True, want_probsum=False):
    """scd_kpp_draw for every row of d2 [R, n] with the uniforms r (host floats [R]).  Returns (idx int64 [R] or None,
    probsum float64 [R] or None)."""
    _need_cuda(d2)
    rr, n = d2.shape
    if torch.is_tensor(r):                                 # already on the device (kpp_lockstep uploads the whole stream once)
        rdev = r.to(device=d2.device, dtype=torch.float32).contiguous()
    else:
        rdev = torch.as_tensor(np.asarray(r, dtype=np.float32)).to(d2.device)
    assert rdev.numel() == rr
    idx = torch.empty(rr, dtype=torch.int64, device=d2.device) if want_idx else None
    ps = torch.empty(rr, dtype=torch.float64, device=d2.device) if want_probsum else None
    nb = rr * _L().scd_kpp_draw_ws_bytes(n)
    ws = _kpp_ws.get((d2.device, nb))
    if ws is None:
        ws = _kpp_ws[(d2.device, nb)] = _ws(nb, d2.device)
    check(_L().scd_kpp_draw_multi(handle(), ptr(d2), n, d2.stride(0), rr, ptr(rdev), ptr(total), ptr(prefix), ptr(idx), ptr(ps),
                                  ptr(ws), nb, stream_ptr()))
    return idx, ps


def kpp_seed_lockstep(x, x16, d2, rv, buf, m0):
    """The rounds of the lock-step k-means++ seeding behind one call (scd_kpp_seed_lockstep): for t < T: draw one row per restart
    from d2 [R, n] with the uniforms rv[t] (float32 [T, R] on the device), store it as centre m0 + t of buf [R, k, d], update d2.
    x16: the exact fp16 copy of x (or None).  Returns the picks, int64 [T, R] on the device (-1: no row drawn)."""
    _need_cuda(x, d2, rv, buf)
    t_rounds, rr = rv.shape
    n, d = x.shape
    assert d2.shape[0] == rr and buf.shape[0] == rr and buf.shape[2] == d and buf.is_contiguous() and rv.is_contiguous()
    picks = torch.empty((t_rounds, rr), dtype=torch.int64, device=x.device)
    nb = _L().scd_kpp_seed_ws_bytes(n, d, rr)
    ws = _kpp_ws.get((x.device, "seed", nb))
    if ws is None:
        ws = _kpp_ws[(x.device, "seed", nb)] = _ws(nb, x.device)
    check(_L().scd_kpp_seed_lockstep(handle(), ptr(x), ptr(x16), n, d, rr, ptr(d2), d2.stride(0), ptr(rv), t_rounds, ptr(buf), buf.shape[1],
                                     int(m0), ptr(picks), ptr(ws), nb, stream_ptr()))
    return picks


def kpp_seed_lockstep_sharded(x, x16, d2, rv, buf, m0, dd):
    """The same rounds over a ROW SHARD behind one call (scd_kpp_seed_lockstep_sharded): the three all-gathers of a round - shard sums,
    shard probability masses, candidate rows - go out through a callback that runs the process group's all-gather on views of one
    exchange buffer.  dd: scd_amd.kmeans._Dist (rank, world, allgather_bytes).  Returns the picks, int64 [T, R] (0, or -1 where no
    shard drew a row)."""
    _need_cuda(x, d2, rv, buf)
    t_rounds, rr = rv.shape
    n, d = x.shape
    assert d2.shape[0] == rr and buf.shape[0] == rr and buf.shape[2] == d and buf.is_contiguous() and rv.is_contiguous()
    dev = x.device
    picks = torch.empty((t_rounds, rr), dtype=torch.int64, device=dev)
    nb = _L().scd_kpp_seed_sharded_ws_bytes(n, d, rr)
    ws = _ws(nb, dev)
    xb = _L().scd_kpp_seed_sharded_xbuf_bytes(d, rr, dd.world)
    xbuf = torch.empty(int(xb), dtype=torch.uint8, device=dev)
    base = xbuf.data_ptr()
    err = []

    def _cb(ctx, send, recv, nbytes, stream):
        # rank w's nbytes at `send` -> recv + w * nbytes on every rank, in stream order (torch's current stream = the kernels' stream)
        try:
            so, ro = send - base, recv - base
            dd.allgather_into(xbuf[ro: ro + dd.world * nbytes], xbuf[so: so + nbytes])
            return 0
        except BaseException as e:            # never unwind through the C frames
            err.append(e)
            return 1
    cb = _lib.GATHER_FN(_cb)
    rc = _L().scd_kpp_seed_lockstep_sharded(handle(), ptr(x), ptr(x16), n, d, rr, ptr(d2), d2.stride(0), ptr(rv), t_rounds, ptr(buf),
                                            buf.shape[1], int(m0), ptr(picks), ptr(ws), nb, stream_ptr(), ptr(xbuf), int(xb), cb, None,
                                            dd.rank, dd.world)
    if err:
        raise err[0]
    check(rc)
    return picks


class UpdateFilter:
    """The distance update of one lock-step seeding round through the MFMA filter (scd_kpp_update_filter), for seedings whose rounds
    are driven from Python (process groups).  One object per seeding: it owns the workspace with the rows' norm table."""

    def __init__(self, x16):
        _need_cuda(x16)
        self.x16 = x16
        self.n, self.d = x16.shape
        self.nb = _L().scd_kpp_update_ws_bytes(self.n, self.d)
        self.ws = _ws(self.nb, x16.device)
        self.first = True

    @staticmethod
    def serves(n, d, restarts):
        dp = (d + 31) // 32 * 32
        return 1 <= restarts <= 16 and d % 32 == 0 and dp in (128, 256, 384, 512, 768)

    def update(self, c_new, d2):
        """d2 [R, ld] = min(d2, ||x - c_new[r]||^2); c_new float32 [R, d] contiguous."""
        assert c_new.dtype == torch.float32 and c_new.is_contiguous() and c_new.shape[1] == self.d and d2.shape[0] == c_new.shape[0]
        check(_L().scd_kpp_update_filter(handle(), ptr(self.x16), self.n, self.d, c_new.shape[0], ptr(c_new), ptr(d2), d2.stride(0),
                                         1 if self.first else 0, ptr(self.ws), self.nb, stream_ptr()))
        self.first = False


def sum_f32_multi(x):
    """float64 row sums of a float32 matrix [R, n] (deterministic order)."""
    _need_cuda(x)
    out = torch.empty(x.shape[0], dtype=torch.float64, device=x.device)
    check(_L().scd_sum_f32_multi(handle(), ptr(x), x.shape[1], x.stride(0), x.shape[0], ptr(out), stream_ptr()))
    return out


def sum_f32(x):
    _need_cuda(x)
    x = x.to(torch.float32).contiguous()
    out = torch.empty(1, dtype=torch.float64, device=x.device)
    check(_L().scd_sum_f32(handle(), ptr(x), x.numel(), ptr(out), stream_ptr()))
    return out


# ----------------------------------------------------------------------------- vote
VOTE_MAX_CLUSTER_ID = 65536         # scd_vote_hist: the cluster slot is a 16-bit field of its sort keys (vote.hip)


def vote_hist(name_idx, top_k, preds, clusters, m, known=None):
    """most_common(m) of every cluster's Counter: (keys int64 [C,m], counts int32 [C,m]); -1/0 padded.
    Limits (the fields of the 64-bit sort keys, scd_vote_hist): cluster ids in [0, 65536) - any other id in `clusters` is refused here,
    a prediction outside it votes for nothing; names in [0, 2^24) - any other name is dropped like a `known` one; n * top_k < 2^24."""
    _need_cuda(name_idx, preds)
    name_idx = name_idx.to(torch.int64).contiguous()
    preds = preds.to(torch.int64).contiguous()
    dev = name_idx.device
    clusters = torch.as_tensor(clusters, dtype=torch.int64).contiguous()
    if clusters.numel() and (int(clusters.min()) < 0 or int(clusters.max()) >= VOTE_MAX_CLUSTER_ID):
        raise _lib.ScdError(_lib.SCD_EINVAL, "vote_hist: cluster ids must lie in [0, %d) (got %d .. %d)"
                            % (VOTE_MAX_CLUSTER_ID, int(clusters.min()), int(clusters.max())))
    clusters = clusters.to(dev)
    kn = None if known is None or len(known) == 0 else torch.as_tensor(known, dtype=torch.int64, device=dev).contiguous()
    n, ld = name_idx.shape
    nc = clusters.numel()
    keys = torch.empty((nc, m), dtype=torch.int64, device=dev)
    counts = torch.empty((nc, m), dtype=torch.int32, device=dev)
    nb = _L().scd_vote_hist_ws_bytes(n, top_k)
    ws = _ws(nb, dev)
    check(_L().scd_vote_hist(handle(), ptr(name_idx), n, ld, top_k, ptr(preds), ptr(clusters), nc, ptr(kn),
                             0 if kn is None else kn.numel(), m, ptr(keys), ptr(counts), ptr(ws), nb, stream_ptr()))
    return keys, counts


def vote_table(name_idx, top_k, preds, clusters, n_slots, row_offset, v):
    """This rank's dense vote tables for its row shard (scd_vote_table): counts int32 [C, V], first int64 [C, V]
    (global first-seen position (row_offset + row) * top_k + column, 0x7f7f7f7f7f7f7f7f = never).  clusters: the cluster ids voted on,
    in table-row order.  Names outside [0, v) and predictions outside [0, n_slots) or not in `clusters` are skipped;
    top_k <= name_idx.shape[1] and (row_offset + n) * top_k < 2^40, or the call is refused."""
    _need_cuda(name_idx, preds)
    name_idx = name_idx.to(torch.int64).contiguous()
    preds = preds.to(torch.int64).contiguous()
    dev = name_idx.device
    nc = len(clusters)
    slot = torch.full((n_slots,), -1, dtype=torch.int32)
    slot[torch.as_tensor(clusters, dtype=torch.int64)] = torch.arange(nc, dtype=torch.int32)
    slot = slot.to(dev)
    counts = torch.empty((nc, v), dtype=torch.int32, device=dev)
    first = torch.empty((nc, v), dtype=torch.int64, device=dev)
    n, ld = name_idx.shape                  # n == 0 (a shard without unlabelled rows) gives empty tables
    check(_L().scd_vote_table(handle(), ptr(name_idx), n, ld, top_k, ptr(preds), ptr(slot), n_slots, int(row_offset), int(v), nc,
                              ptr(counts), ptr(first), stream_ptr()))
    return counts, first


def vote_table_topm(counts, first, m):
    """most_common(m) per cluster from the (all-reduced) tables: (keys int64 [C, m], counts int32 [C, m]); -1 / 0 padded.
    Order: count descending (any int32 count, up to 2^31 - 1), then `first` ascending (all 64 bits).  SIDE EFFECT: the cells it
    takes are set to 0 in `counts`; every other cell and `first` stay as they are - pass a clone to keep the table."""
    _need_cuda(counts, first)
    nc, v = counts.shape
    keys = torch.empty((nc, m), dtype=torch.int64, device=counts.device)
    cnt = torch.empty((nc, m), dtype=torch.int32, device=counts.device)
    check(_L().scd_vote_table_topm(handle(), ptr(counts), ptr(first), nc, v, m, ptr(keys), ptr(cnt), stream_ptr()))
    return keys, cnt


# ----------------------------------------------------------------------------- clustering scores
def contingency_private_cells():
    """The largest S * kp * kt for which scd_contingency counts in per-block LDS tables (above it: one global add per row)."""
    return int(_L().scd_contingency_private_cells())


def contingency(pred, truth, subset, kp, kt):
    """scd_contingency: pred, truth int32 [n] and subset uint8 [n] or None on the device -> (table int32 [S, kp, kt], n_bad int64 [1]),
    S = 1 without subset, else 2 (table 0: rows with subset != 0).  Rows with a label outside the table are counted in n_bad only."""
    _need_cuda(pred, truth, subset)
    if pred.dtype != torch.int32 or truth.dtype != torch.int32 or (subset is not None and subset.dtype != torch.uint8):
        raise _lib.ScdError(_lib.SCD_EINVAL, "contingency: pred / truth must be int32 and subset uint8")
    pred, truth = pred.contiguous(), truth.contiguous()
    subset = None if subset is None else subset.contiguous()
    n = pred.numel()
    if truth.numel() != n or (subset is not None and subset.numel() != n):
        raise _lib.ScdError(_lib.SCD_EINVAL, "contingency: pred, truth and subset must have one length")
    s = 1 if subset is None else 2
    table = torch.empty((s, int(kp), int(kt)), dtype=torch.int32, device=pred.device)
    n_bad = torch.empty(1, dtype=torch.int64, device=pred.device)
    check(_L().scd_contingency(handle(), ptr(pred), ptr(truth), ptr(subset), n, int(kp), int(kt), ptr(table), ptr(n_bad), stream_ptr()))
    return table, n_bad


def contingency_last_path():
    """0: the last contingency() counted in per-block LDS tables, 1: with one global add per row (-1 before the first call)."""
    return int(_L().scd_contingency_last_path(handle()))


def contingency_stats(table):
    """scd_contingency_stats of table int32 [S, kp, kt]: (ints int64 [S, 6] = n, sum n_ij^2, sum a_i^2, sum b_j^2, sum_i max_j n_ij,
    non-zero cells; info float64 [S, 3] = H(pred), H(truth), MI in nats) on the device."""
    _need_cuda(table)
    if table.dtype != torch.int32 or table.dim() != 3:
        raise _lib.ScdError(_lib.SCD_EINVAL, "contingency_stats: table must be int32 [S, kp, kt]")
    table = table.contiguous()
    s, kp, kt = table.shape
    ints = torch.empty((s, 6), dtype=torch.int64, device=table.device)
    info = torch.empty((s, 3), dtype=torch.float64, device=table.device)
    nb = _L().scd_contingency_stats_ws_bytes(s, kp, kt)
    ws = _ws(nb, table.device)
    check(_L().scd_contingency_stats(handle(), ptr(table), s, kp, kt, ptr(ints), ptr(info), ptr(ws), nb, stream_ptr()))
    return ints, info


def silhouette(x, labels, k):
    """scd_silhouette: x fp16 / fp32 [n, d] and labels int32 [n] on the device -> (samples float32 [n] in x's row order, mean float64
    [1], info int64 [2] = rows with a label outside [0, k), non-empty clusters), all on the device.  Fewer than two non-empty clusters
    give zeros; the callers in scd_amd.metrics raise on that and on a bad label."""
    _need_cuda(x, labels)
    if x.dim() != 2 or x.dtype not in (torch.float16, torch.float32) or labels.dtype != torch.int32:
        raise _lib.ScdError(_lib.SCD_EINVAL, "silhouette: x must be fp16 / fp32 [n, d] and labels int32")
    x, labels = x.contiguous(), labels.contiguous()
    n, d = x.shape
    if labels.numel() != n:
        raise _lib.ScdError(_lib.SCD_EINVAL, "silhouette: x and labels must have one length")
    samples = torch.empty(n, dtype=torch.float32, device=x.device)
    mean = torch.empty(1, dtype=torch.float64, device=x.device)
    info = torch.empty(2, dtype=torch.int64, device=x.device)
    nb = _L().scd_silhouette_ws_bytes(n, d, int(k))
    ws = _ws(max(nb, 16), x.device)
    dt = SCD_F32 if x.dtype == torch.float32 else SCD_F16
    check(_L().scd_silhouette(handle(), ptr(x), dt, ptr(labels), n, d, int(k), ptr(samples), ptr(mean), ptr(info), ptr(ws), nb, stream_ptr()))
    return samples, mean, info


def silhouette_ranges(n, k):
    """scd_silhouette_ranges: the number of cluster ranges (grid.y) silhouette() launches with for n rows and k ids on this device
    (0 outside the kernel's limits).  The samples do not depend on it; tests size their cases with it."""
    return int(_L().scd_silhouette_ranges(handle(), int(n), int(k)))


# ----------------------------------------------------------------------------- FINCH primitives (docs/design/finch.md)
def first_neighbor(u):
    """scd_first_neighbor: u float32 [n, d] on the device -> (nn int32 [n], d1 float64 [n], info int32 [2] = rows through the exact
    full-row pass, fp16-overflow flag), all on the device.  nn[i] = argmax over j != i of the float64 dot of rows i and j, ties to the
    lowest j; d1 = 1 - that dot."""
    _need_cuda(u)
    if u.dim() != 2 or u.dtype != torch.float32:
        raise _lib.ScdError(_lib.SCD_EINVAL, "first_neighbor: u must be float32 [n, d]")
    u = u.contiguous()
    n, d = u.shape
    nn = torch.empty(n, dtype=torch.int32, device=u.device)
    d1 = torch.empty(n, dtype=torch.float64, device=u.device)
    info = torch.empty(2, dtype=torch.int32, device=u.device)
    nb = _L().scd_first_neighbor_ws_bytes(n, d)
    ws = _ws(max(nb, 16), u.device)
    check(_L().scd_first_neighbor(handle(), ptr(u), n, d, ptr(nn), ptr(d1), ptr(info), ptr(ws), nb, stream_ptr()))
    return nn, d1, info


def pair_dist_f64(u, a, b):
    """scd_pair_dist_f64: 1 - float64 dot of rows a[p] and b[p] of u float32 [n, d]; a, b int32 [m] on the device -> float64 [m]."""
    _need_cuda(u, a, b)
    if u.dim() != 2 or u.dtype != torch.float32 or a.dtype != torch.int32 or b.dtype != torch.int32 or a.numel() != b.numel():
        raise _lib.ScdError(_lib.SCD_EINVAL, "pair_dist_f64: u must be float32 [n, d], a and b int32 of one length")
    u, a, b = u.contiguous(), a.contiguous(), b.contiguous()
    out = torch.empty(a.numel(), dtype=torch.float64, device=u.device)
    check(_L().scd_pair_dist_f64(handle(), ptr(u), u.shape[0], u.shape[1], ptr(a), ptr(b), a.numel(), ptr(out), stream_ptr()))
    return out


def link_components(n, ea, eb):
    """scd_link_components: the connected components of the undirected edges (ea[e], eb[e]) (device int32 [m]) on n nodes ->
    (labels int32 [n] numbered by the rank of each component's lowest member, the number of components as an int)."""
    _need_cuda(ea, eb)
    if ea.dtype != torch.int32 or eb.dtype != torch.int32 or ea.numel() != eb.numel():
        raise _lib.ScdError(_lib.SCD_EINVAL, "link_components: ea and eb must be int32 of one length")
    ea, eb = ea.contiguous(), eb.contiguous()
    labels = torch.empty(int(n), dtype=torch.int32, device=ea.device)
    ncomp = torch.empty(1, dtype=torch.int32, device=ea.device)
    nb = _L().scd_link_components_ws_bytes(int(n))
    ws = _ws(max(nb, 16), ea.device)
    check(_L().scd_link_components(handle(), int(n), ptr(ea), ptr(eb), ea.numel(), ptr(labels), ptr(ncomp), ptr(ws), nb, stream_ptr()))
    return labels, int(ncomp.item())


def segment_mean_unit(x, order, offsets):
    """scd_segment_mean_unit: x float32 [n, d], order int32 [n] (the stable sort of the rows by label), offsets int64 [k + 1] ->
    (means float32 [k, d]: float64 sums in row order / count; their unit rows float32 [k, d], the norm in float64)."""
    _need_cuda(x, order, offsets)
    if x.dim() != 2 or x.dtype != torch.float32 or order.dtype != torch.int32 or offsets.dtype != torch.int64 or offsets.numel() < 2:
        raise _lib.ScdError(_lib.SCD_EINVAL, "segment_mean_unit: x float32 [n, d], order int32, offsets int64 [k + 1]")
    x, order, offsets = x.contiguous(), order.contiguous(), offsets.contiguous()
    k, d = offsets.numel() - 1, x.shape[1]
    if order.numel() != x.shape[0]:
        raise _lib.ScdError(_lib.SCD_EINVAL, "segment_mean_unit: order must hold one entry per row of x")
    mean = torch.empty((k, d), dtype=torch.float32, device=x.device)
    unit = torch.empty((k, d), dtype=torch.float32, device=x.device)
    check(_L().scd_segment_mean_unit(handle(), ptr(x), x.shape[0], ptr(order), ptr(offsets), k, d, ptr(mean), ptr(unit), stream_ptr()))
    return mean, unit


# ----------------------------------------------------------------------------- exact k nearest neighbours (docs/design/knn.md)
def knn(q, x, k, self_base=-1):
    """scd_knn: queries q float32 [m, d] and base rows x float32 [n, d] on the device -> (idx int32 [m, k], dot float64 [m, k], info
    int32 [4] = rows through the exact full-row pass, fp16-overflow flag, rows whose candidate slots overflowed, largest candidate
    count), all on the device.  Row i: the k columns j != self_base + i with the largest float64 dot, ordered by (dot descending,
    column ascending).  self_base = -1 excludes nothing; q a view of rows a .. a + m of x with self_base = a is a shard of the graph."""
    _need_cuda(q, x)
    if q.dim() != 2 or x.dim() != 2 or q.dtype != torch.float32 or x.dtype != torch.float32 or q.shape[1] != x.shape[1]:
        raise _lib.ScdError(_lib.SCD_EINVAL, "knn: q and x must be float32 [m, d] and [n, d]")
    q, x = q.contiguous(), x.contiguous()
    (m, d), n, k = q.shape, x.shape[0], int(k)
    idx = torch.empty((m, max(k, 0)), dtype=torch.int32, device=x.device)
    dot = torch.empty((m, max(k, 0)), dtype=torch.float64, device=x.device)
    info = torch.empty(4, dtype=torch.int32, device=x.device)
    nb = _L().scd_knn_ws_bytes(m, n, d, k)
    ws = _ws(max(nb, 16), x.device)
    check(_L().scd_knn(handle(), ptr(q), m, ptr(x), n, d, k, int(self_base), ptr(idx), ptr(dot), ptr(info), ptr(ws), nb, stream_ptr()))
    return idx, dot, info


KNN_UNIFORM, KNN_SOFTMAX = 0, 1


def knn_vote(idx, dot, base_labels, k_use=None, mode=KNN_SOFTMAX, temperature=0.07):
    """scd_knn_vote: idx int32 [m, k] and dot float64 [m, k] as `knn` returns them, base_labels int32 [n] -> (pred int32 [m], score
    float64 [m]).  The first k_use neighbours vote: KNN_UNIFORM counts, KNN_SOFTMAX weights exp((dot_j - dot_0) / temperature); the
    largest class score wins, ties to the lowest class; negative labels do not vote and a query without a vote gets -1."""
    _need_cuda(idx, dot, base_labels)
    if idx.dim() != 2 or idx.shape != dot.shape or idx.dtype != torch.int32 or dot.dtype != torch.float64 or base_labels.dtype != torch.int32:
        raise _lib.ScdError(_lib.SCD_EINVAL, "knn_vote: idx int32 [m, k], dot float64 [m, k], base_labels int32 [n]")
    idx, dot, base_labels = idx.contiguous(), dot.contiguous(), base_labels.contiguous()
    m, k = idx.shape
    k_use = k if k_use is None else int(k_use)
    pred = torch.empty(m, dtype=torch.int32, device=idx.device)
    score = torch.empty(m, dtype=torch.float64, device=idx.device)
    check(_L().scd_knn_vote(handle(), ptr(idx), ptr(dot), m, k, k_use, ptr(base_labels), base_labels.numel(), int(mode), float(temperature),
                            ptr(pred), ptr(score), stream_ptr()))
    return pred, score


# ----------------------------------------------------------------------------- HDBSCAN primitives (docs/design/hdbscan.md)
def mr_nearest_workspace(u):
    """The workspace of `mr_nearest` for u float32 [n, d]: allocate once per fit and pass it to every round, so that the fp16 copy of u is
    made once (the first call with prepared=False)."""
    _need_cuda(u)
    if u.dim() != 2 or u.dtype != torch.float32:
        raise _lib.ScdError(_lib.SCD_EINVAL, "mr_nearest: u must be float32 [n, d]")
    nb = _L().scd_mr_nearest_ws_bytes(u.shape[0], u.shape[1])
    if nb == 0:
        raise _lib.ScdError(_lib.SCD_EINVAL, "mr_nearest: n = %d, d = %d outside the limits 2 <= n < 2^31, d <= 1024" % tuple(u.shape))
    return _ws(nb, u.device)


def mr_nearest(u, core, comp, ws=None, prepared=False):
    """scd_mr_nearest, one Boruvka round: u float32 [n, d], core float64 [n] (core dots, +inf allowed), comp int32 [n] on the device ->
    (nn int32 [n], r float64 [n], info int32 [4]).  nn[i] = the column j with comp[j] != comp[i] of the largest min(core_i, core_j,
    float64 dot of rows i and j), ties to the lowest j; r[i] = that value; -1 and -inf for a row without a foreign column.
    ws: `mr_nearest_workspace(u)`; prepared=True says it still holds this u's fp16 copy from an earlier call."""
    _need_cuda(u, core, comp)
    if u.dim() != 2 or u.dtype != torch.float32 or core.dtype != torch.float64 or comp.dtype != torch.int32 \
            or core.shape != (u.shape[0],) or comp.shape != (u.shape[0],):
        raise _lib.ScdError(_lib.SCD_EINVAL, "mr_nearest: u float32 [n, d], core float64 [n], comp int32 [n]")
    if not u.is_contiguous():
        raise _lib.ScdError(_lib.SCD_EINVAL, "mr_nearest: u must be contiguous (the workspace's copy belongs to this tensor)")
    core, comp = core.contiguous(), comp.contiguous()
    n, d = u.shape
    if ws is None:
        ws, prepared = mr_nearest_workspace(u), False
    nn = torch.empty(n, dtype=torch.int32, device=u.device)
    r = torch.empty(n, dtype=torch.float64, device=u.device)
    info = torch.empty(4, dtype=torch.int32, device=u.device)
    check(_L().scd_mr_nearest(handle(), ptr(u), n, d, ptr(core), ptr(comp), 1 if prepared else 0, ptr(nn), ptr(r), ptr(info), ptr(ws),
                              ws.numel(), stream_ptr()))
    return nn, r, info


# ----------------------------------------------------------------------------- Ward primitives (docs/design/ward.md)
WARD_WS_CAP = 2 << 30           # a fit's workspace stays under 2 GiB: 126,976 x 768 needs 0.68 GB


def ward_workspace(q, m, d, device):
    """The workspace of `ward_nearest` for up to q queries against a table of m positions of d columns: allocate once per fit; the table's
    part (the fp16 copy, row statistics and norms) is kept between calls and refreshed by `ward_merge`."""
    nb = _L().scd_ward_nearest_ws_bytes(int(q), int(m), int(d))
    if nb == 0:
        raise _lib.ScdError(_lib.SCD_EINVAL, "ward_nearest: q = %d, m = %d, d = %d outside the limits 1 <= q < 2^29, 2 <= m < 2^29, d <= 1024"
                            % (q, m, d))
    if nb > WARD_WS_CAP:
        raise _lib.ScdError(_lib.SCD_EINVAL, "ward_nearest: the workspace for q = %d, m = %d, d = %d is %d bytes, over the 2 GiB cap"
                            % (q, m, d, nb))
    return _ws(nb, device)


def ward_nearest(q, qcnt, qself, x, xcnt, ws=None, prepared=0):
    """scd_ward_nearest: queries q float32 [nq, d] with sizes qcnt int32 [nq] and own columns qself int32 [nq] (-1: none) against the
    table x float32 [m, d] with sizes xcnt int32 [m] (0: dead), all on the device -> (nn int32 [nq], cost float64 [nq], info int32 [4]).
    nn[p] = the live column j != qself[p] of the least Ward cost, ties to the lowest j; -1 and +inf for a query without one.
    ws: `ward_workspace(nq, m, d, device)` or larger in q; prepared: how many leading positions of x it still holds."""
    _need_cuda(q, qcnt, qself, x, xcnt)
    if q.dim() != 2 or x.dim() != 2 or q.dtype != torch.float32 or x.dtype != torch.float32 or q.shape[1] != x.shape[1] \
            or qcnt.dtype != torch.int32 or qself.dtype != torch.int32 or xcnt.dtype != torch.int32 \
            or qcnt.shape != (q.shape[0],) or qself.shape != (q.shape[0],) or xcnt.shape != (x.shape[0],):
        raise _lib.ScdError(_lib.SCD_EINVAL, "ward_nearest: q float32 [nq, d], qcnt, qself int32 [nq], x float32 [m, d], xcnt int32 [m]")
    if not x.is_contiguous() or not xcnt.is_contiguous():
        raise _lib.ScdError(_lib.SCD_EINVAL, "ward_nearest: x and xcnt must be contiguous (the workspace's copy belongs to this table)")
    q, qcnt, qself = q.contiguous(), qcnt.contiguous(), qself.contiguous()
    (nq, d), m = q.shape, x.shape[0]
    if ws is None:
        ws, prepared = ward_workspace(nq, m, d, x.device), 0
    nn = torch.empty(nq, dtype=torch.int32, device=x.device)
    cost = torch.empty(nq, dtype=torch.float64, device=x.device)
    info = torch.empty(4, dtype=torch.int32, device=x.device)
    check(_L().scd_ward_nearest(handle(), ptr(q), ptr(qcnt), ptr(qself), ptr(x), ptr(xcnt), nq, m, d, int(prepared), ptr(nn), ptr(cost),
                                ptr(info), ptr(ws), ws.numel(), stream_ptr()))
    return nn, cost, info


def ward_merge(x, xcnt, lo, hi, ws):
    """scd_ward_merge, in place: the pairs (lo[e], hi[e]) int32 of one round, lo < hi, no position twice.  x[lo] becomes the weighted
    centroid, xcnt[lo] the sum, xcnt[hi] = 0, and the workspace's data of position lo is made again."""
    _need_cuda(x, xcnt, lo, hi, ws)
    if x.dim() != 2 or x.dtype != torch.float32 or xcnt.dtype != torch.int32 or xcnt.shape != (x.shape[0],) or lo.dtype != torch.int32 \
            or hi.dtype != torch.int32 or lo.dim() != 1 or lo.shape != hi.shape:
        raise _lib.ScdError(_lib.SCD_EINVAL, "ward_merge: x float32 [m, d], xcnt int32 [m], lo and hi int32 [pairs]")
    if not (x.is_contiguous() and xcnt.is_contiguous()):
        raise _lib.ScdError(_lib.SCD_EINVAL, "ward_merge: x and xcnt are changed in place and must be contiguous")
    lo, hi = lo.contiguous(), hi.contiguous()
    check(_L().scd_ward_merge(handle(), ptr(x), ptr(xcnt), ptr(lo), ptr(hi), lo.numel(), x.shape[0], x.shape[1], ptr(ws), ws.numel(),
                              stream_ptr()))


HDBSCAN_METHODS = {"eom": 0, "leaf": 1}


def hdbscan_tree(lo, hi, weight, min_cluster_size, method="eom", allow_single_cluster=False):
    """scd_hdbscan_tree (host): the n - 1 sorted edges (lo, hi, weight) of a spanning tree -> (labels int64 [n] with noise = -1,
    probabilities float64 [n], the number of clusters): scikit-learn's make_single_linkage + tree_to_labels."""
    lo = np.ascontiguousarray(lo, dtype=np.int32)
    hi = np.ascontiguousarray(hi, dtype=np.int32)
    w = np.ascontiguousarray(weight, dtype=np.float64)
    if method not in HDBSCAN_METHODS:
        raise _lib.ScdError(_lib.SCD_EINVAL, "hdbscan_tree: cluster_selection_method %r is not one of %s" % (method, sorted(HDBSCAN_METHODS)))
    if not (lo.ndim == hi.ndim == w.ndim == 1 and lo.size == hi.size == w.size):
        raise _lib.ScdError(_lib.SCD_EINVAL, "hdbscan_tree: lo, hi and weight must be vectors of one length")
    n = lo.size + 1
    labels = np.empty(n, dtype=np.int32)
    prob = np.empty(n, dtype=np.float64)
    nclu = C.c_int32(0)
    check(_L().scd_hdbscan_tree(ptr(lo), ptr(hi), ptr(w), n, int(min_cluster_size), HDBSCAN_METHODS[method], 1 if allow_single_cluster else 0,
                                ptr(labels), ptr(prob), C.byref(nclu)))
    return labels.astype(np.int64), prob, int(nclu.value)


# ----------------------------------------------------------------------------- the linear probe (docs/design/probe.md)
def _probe_args(who, x, w, b):
    _need_cuda(x, w)
    if x.dim() != 2 or w.dim() != 2 or x.dtype != torch.float32 or w.dtype != torch.float32 or x.shape[1] != w.shape[1]:
        raise _lib.ScdError(_lib.SCD_EINVAL, who + ": x float32 [n, d] and w float32 [c, d]")
    if b is not None:
        _need_cuda(b)
        if b.dtype != torch.float32 or b.shape != (w.shape[0],):
            raise _lib.ScdError(_lib.SCD_EINVAL, who + ": b float32 [c]")
        b = b.contiguous()
    return x.contiguous(), w.contiguous(), b


def probe_loss_grad(x, y, w, b=None, sample_weight=None, want_pred=False):
    """scd_probe_loss_grad: x float32 [n, d], y int32 [n], w float32 [c, d], b float32 [c] or None, sample_weight float32 [n] or None ->
    (loss float64 [1], gw float64 [c, d], gb float64 [c] or None without b, pred int32 [n] or None, info int32 [2] = rows with a label
    outside [0, c), rows with a non-finite logit), all on the device.  The data term sum_i s_i [lse(z_i) - z_{i, y_i}] of multinomial
    logistic regression and its gradient; the L2 term is the caller's."""
    x, w, b = _probe_args("probe_loss_grad", x, w, b)
    _need_cuda(y)
    (n, d), c = x.shape, w.shape[0]
    if y.dtype != torch.int32 or y.shape != (n,):
        raise _lib.ScdError(_lib.SCD_EINVAL, "probe_loss_grad: y int32 [n]")
    y = y.contiguous()
    if sample_weight is not None:
        _need_cuda(sample_weight)
        if sample_weight.dtype != torch.float32 or sample_weight.shape != (n,):
            raise _lib.ScdError(_lib.SCD_EINVAL, "probe_loss_grad: sample_weight float32 [n]")
        sample_weight = sample_weight.contiguous()
    loss = torch.empty(1, dtype=torch.float64, device=x.device)
    gw = torch.empty((c, d), dtype=torch.float64, device=x.device)
    gb = torch.empty(c, dtype=torch.float64, device=x.device) if b is not None else None
    pred = torch.empty(n, dtype=torch.int32, device=x.device) if want_pred else None
    info = torch.empty(2, dtype=torch.int32, device=x.device)
    nb = _L().scd_probe_ws_bytes(n, d, c)
    ws = _ws(max(nb, 16), x.device)
    check(_L().scd_probe_loss_grad(handle(), ptr(x), ptr(y), ptr(sample_weight), n, d, c, ptr(w), ptr(b), ptr(loss), ptr(gw), ptr(gb),
                                   ptr(pred), ptr(info), ptr(ws), nb, stream_ptr()))
    return loss, gw, gb, pred, info


def probe_predict(x, w, b=None, want_top=False):
    """scd_probe_predict: x float32 [n, d], w float32 [c, d], b float32 [c] or None -> pred int32 [n] = argmax_c (w_c . x_i + b_c), ties to
    the lowest class; with want_top also top float32 [n, 2], the largest and second largest logit of each row."""
    x, w, b = _probe_args("probe_predict", x, w, b)
    (n, d), c = x.shape, w.shape[0]
    pred = torch.empty(n, dtype=torch.int32, device=x.device)
    top = torch.empty((n, 2), dtype=torch.float32, device=x.device) if want_top else None
    nb = _L().scd_probe_ws_bytes(1, d, c)
    ws = _ws(max(nb, 16), x.device)
    check(_L().scd_probe_predict(handle(), ptr(x), n, d, c, ptr(w), ptr(b), ptr(pred), ptr(top), ptr(ws), nb, stream_ptr()))
    return (pred, top) if want_top else pred


# ----------------------------------------------------------------------------- Gaussian mixtures (docs/design/gmm.md)
def _gmm_params(who, x, a, b, c):
    _need_cuda(x, a, b, c)
    if x.dim() != 2 or x.dtype != torch.float32:
        raise _lib.ScdError(_lib.SCD_EINVAL, who + ": x float32 [n, d]")
    k, d = a.shape[0] if a.dim() == 1 else -1, x.shape[1]
    if any(t.dtype != torch.float32 for t in (a, b, c)) or k < 1 or b.shape != (k, d) or c.shape != (k, d):
        raise _lib.ScdError(_lib.SCD_EINVAL, who + ": a float32 [k], b and c float32 [k, d]")
    return x.contiguous(), a.contiguous(), b.contiguous(), c.contiguous()


def gmm_em_step(x, a, b, c, y=None, sample_weight=None, want_pred=False, n_components=None):
    """scd_gmm_em_step: x float32 [n, d]; a float32 [k], b = mu / v and c = -1 / (2 v) float32 [k, d] (the weighted log-density
    z_ik = a_k + x_i . b_k + x_i^2 . c_k); y int32 [n] or None (a row with 0 <= y_i < k is clamped to its class, any other is
    unlabelled); sample_weight float32 [n] or None -> (ll float64 [1], nk float64 [k], s1 float64 [k, d] = r^T x, s2 float64 [k, d] =
    r^T x^2, pred int32 [n] or None, info int32 [2] = rows with y_i >= k, rows with a non-finite logit), all on the device.
    With a = b = c = None and n_components = k it is the hard M-step: the labelled rows' one-hots alone, ll = 0, no pred."""
    hard = a is None and b is None and c is None
    if hard:
        _need_cuda(x)
        if x.dim() != 2 or x.dtype != torch.float32 or n_components is None or int(n_components) < 1 or y is None or want_pred:
            raise _lib.ScdError(_lib.SCD_EINVAL, "gmm_em_step: the hard M-step takes x float32 [n, d], y, n_components >= 1 and no pred")
        x, k = x.contiguous(), int(n_components)
    else:
        if a is None or b is None or c is None:
            raise _lib.ScdError(_lib.SCD_EINVAL, "gmm_em_step: a, b and c are all given or all None")
        x, a, b, c = _gmm_params("gmm_em_step", x, a, b, c)
        k = a.shape[0]
    n, d = x.shape
    if y is not None:
        _need_cuda(y)
        if y.dtype != torch.int32 or y.shape != (n,):
            raise _lib.ScdError(_lib.SCD_EINVAL, "gmm_em_step: y int32 [n]")
        y = y.contiguous()
    if sample_weight is not None:
        _need_cuda(sample_weight)
        if sample_weight.dtype != torch.float32 or sample_weight.shape != (n,):
            raise _lib.ScdError(_lib.SCD_EINVAL, "gmm_em_step: sample_weight float32 [n]")
        sample_weight = sample_weight.contiguous()
    ll = torch.empty(1, dtype=torch.float64, device=x.device)
    nk = torch.empty(k, dtype=torch.float64, device=x.device)
    s1 = torch.empty((k, d), dtype=torch.float64, device=x.device)
    s2 = torch.empty((k, d), dtype=torch.float64, device=x.device)
    pred = torch.empty(n, dtype=torch.int32, device=x.device) if want_pred else None
    info = torch.empty(2, dtype=torch.int32, device=x.device)
    nb = _L().scd_gmm_ws_bytes(n, d, k)
    ws = _ws(max(nb, 16), x.device)
    check(_L().scd_gmm_em_step(handle(), ptr(x), ptr(y), ptr(sample_weight), n, d, k, ptr(a), ptr(b), ptr(c), ptr(ll), ptr(nk), ptr(s1),
                               ptr(s2), ptr(pred), ptr(info), ptr(ws), nb, stream_ptr()))
    return ll, nk, s1, s2, pred, info


def gmm_predict(x, a, b, c, want_ll=False, want_resp=False):
    """scd_gmm_predict: x float32 [n, d], a float32 [k], b and c float32 [k, d] -> (pred int32 [n] = argmax_k z_ik, ties to the lowest
    component; row_ll float32 [n] = lse_k z_ik or None; resp float32 [n, k] = softmax_k(z_i) or None)."""
    x, a, b, c = _gmm_params("gmm_predict", x, a, b, c)
    (n, d), k = x.shape, a.shape[0]
    pred = torch.empty(n, dtype=torch.int32, device=x.device)
    row_ll = torch.empty(n, dtype=torch.float32, device=x.device) if want_ll else None
    resp = torch.empty((n, k), dtype=torch.float32, device=x.device) if want_resp else None
    nb = _L().scd_gmm_ws_bytes(1, d, k)
    ws = _ws(max(nb, 16), x.device)
    check(_L().scd_gmm_predict(handle(), ptr(x), n, d, k, ptr(a), ptr(b), ptr(c), ptr(pred), ptr(row_ll), ptr(resp), ptr(ws), nb,
                               stream_ptr()))
    return pred, row_ll, resp


# ----------------------------------------------------------------------------- full-covariance mixtures (docs/design/gmm_full.md)
def _gmm_full_params(who, x, a, mu, ut):
    _need_cuda(x, a, mu, ut)
    if x.dim() != 2 or x.dtype != torch.float32:
        raise _lib.ScdError(_lib.SCD_EINVAL, who + ": x float32 [n, d]")
    k, d = a.shape[0] if a.dim() == 1 else -1, x.shape[1]
    if any(t.dtype != torch.float32 for t in (a, mu, ut)) or k < 1 or mu.shape != (k, d) or ut.shape != (k, d, d):
        raise _lib.ScdError(_lib.SCD_EINVAL, who + ": a float32 [k], mu float32 [k, d], ut float32 [k, d, d]")
    return x.contiguous(), a.contiguous(), mu.contiguous(), ut.contiguous()


def gmm_full_em_step(x, a, mu, ut, y=None, sample_weight=None, want_pred=False):
    """scd_gmm_full_em_step: x float32 [n, d <= 64]; a float32 [k], mu float32 [k, d], ut float32 [k, d, d] with ut[k, j, l] =
    U_k[l, j] (U_k the upper-triangular precision factor; z_ik = a_k - 0.5 |(x_i - mu_k) U_k|^2); y int32 [n] or None (a row with
    0 <= y_i < k is clamped to its class); sample_weight float32 [n] or None -> (ll float64 [1], nk float64 [k], s1c float64 [k, d] =
    sum_i r_ik (x_i - mu_k), S float64 [k, d, d] = sum_i r_ik (x_i - mu_k)(x_i - mu_k)^T, pred int32 [n] or None, info int32 [2]), all
    on the device.  With a = ut = None it is the hard M-step about the centres mu: the labelled rows' one-hots alone, ll = 0, no pred."""
    hard = a is None and ut is None
    if hard:
        _need_cuda(x, mu)
        if (x.dim() != 2 or x.dtype != torch.float32 or mu is None or mu.dtype != torch.float32 or mu.dim() != 2 or mu.shape[0] < 1
                or mu.shape[1] != x.shape[1] or y is None or want_pred):
            raise _lib.ScdError(_lib.SCD_EINVAL, "gmm_full_em_step: the hard M-step takes x float32 [n, d], mu float32 [k, d], y and no pred")
        x, mu = x.contiguous(), mu.contiguous()
    else:
        if a is None or ut is None or mu is None:
            raise _lib.ScdError(_lib.SCD_EINVAL, "gmm_full_em_step: a and ut are both given or both None")
        x, a, mu, ut = _gmm_full_params("gmm_full_em_step", x, a, mu, ut)
    (n, d), k = x.shape, mu.shape[0]
    if y is not None:
        _need_cuda(y)
        if y.dtype != torch.int32 or y.shape != (n,):
            raise _lib.ScdError(_lib.SCD_EINVAL, "gmm_full_em_step: y int32 [n]")
        y = y.contiguous()
    if sample_weight is not None:
        _need_cuda(sample_weight)
        if sample_weight.dtype != torch.float32 or sample_weight.shape != (n,):
            raise _lib.ScdError(_lib.SCD_EINVAL, "gmm_full_em_step: sample_weight float32 [n]")
        sample_weight = sample_weight.contiguous()
    ll = torch.empty(1, dtype=torch.float64, device=x.device)
    nk = torch.empty(k, dtype=torch.float64, device=x.device)
    s1c = torch.empty((k, d), dtype=torch.float64, device=x.device)
    S = torch.empty((k, d, d), dtype=torch.float64, device=x.device)
    pred = torch.empty(n, dtype=torch.int32, device=x.device) if want_pred else None
    info = torch.empty(2, dtype=torch.int32, device=x.device)
    nb = _L().scd_gmm_full_ws_bytes(n, d, k)
    ws = _ws(max(nb, 16), x.device)
    check(_L().scd_gmm_full_em_step(handle(), ptr(x), ptr(y), ptr(sample_weight), n, d, k, ptr(a), ptr(mu), ptr(ut), ptr(ll), ptr(nk),
                                    ptr(s1c), ptr(S), ptr(pred), ptr(info), ptr(ws), nb, stream_ptr()))
    return ll, nk, s1c, S, pred, info


def gmm_full_predict(x, a, mu, ut, want_ll=False, want_resp=False):
    """scd_gmm_full_predict: x float32 [n, d <= 64], a float32 [k], mu float32 [k, d], ut float32 [k, d, d] -> (pred int32 [n], ties to
    the lowest component; row_ll float32 [n] = lse_k z_ik or None; resp float32 [n, k] = softmax_k(z_i) or None)."""
    x, a, mu, ut = _gmm_full_params("gmm_full_predict", x, a, mu, ut)
    (n, d), k = x.shape, a.shape[0]
    pred = torch.empty(n, dtype=torch.int32, device=x.device)
    row_ll = torch.empty(n, dtype=torch.float32, device=x.device) if want_ll else None
    resp = torch.empty((n, k), dtype=torch.float32, device=x.device) if want_resp else None
    nb = _L().scd_gmm_full_ws_bytes(1, d, k)
    ws = _ws(max(nb, 16), x.device)
    check(_L().scd_gmm_full_predict(handle(), ptr(x), n, d, k, ptr(a), ptr(mu), ptr(ut), ptr(pred), ptr(row_ll), ptr(resp), ptr(ws), nb,
                                    stream_ptr()))
    return pred, row_ll, resp


# ----------------------------------------------------------------------------- principal components (docs/design/pca.md)
def _pca_args(who, x, shift):
    _need_cuda(x, shift)
    if x.dim() != 2 or x.dtype != torch.float32 or x.shape[0] < 1 or x.shape[1] < 1:
        raise _lib.ScdError(_lib.SCD_EINVAL, who + ": x float32 [n, d]")
    if shift is not None:
        if shift.dtype != torch.float32 or shift.shape != (x.shape[1],):
            raise _lib.ScdError(_lib.SCD_EINVAL, who + ": shift float32 [d] or None")
        shift = shift.contiguous()
    return x.contiguous(), shift


def _pca_ws(who, n, d, m, device):
    nb = _L().scd_pca_ws_bytes(n, d, m)
    if nb == 0:
        raise _lib.ScdError(_lib.SCD_EINVAL, "%s: outside the limits 1 <= n < 2^31, 1 <= d <= 1024, 1 <= m <= 1024 (n = %d, d = %d, m = %d)"
                            % (who, n, d, m))
    return _ws(nb, device), nb


def pca_colsum(x, shift=None):
    """scd_pca_colsum: x float32 [n, d], shift float32 [d] or None -> csum float64 [d] = sum_i fl32(x_ij - shift_j), on the device."""
    x, shift = _pca_args("pca_colsum", x, shift)
    n, d = x.shape
    csum = torch.empty(d, dtype=torch.float64, device=x.device)
    ws, nb = _pca_ws("pca_colsum", n, d, 1, x.device)
    check(_L().scd_pca_colsum(handle(), ptr(x), ptr(shift), n, d, ptr(csum), ptr(ws), nb, stream_ptr()))
    return csum


def pca_gram(x, shift=None):
    """scd_pca_gram: x float32 [n, d], shift float32 [d] or None -> (G float64 [d, d] = c^T c with c = fl32(x - shift), bit-symmetric;
    info int32 [2] = rows that hold a non-finite value, 0), on the device."""
    x, shift = _pca_args("pca_gram", x, shift)
    n, d = x.shape
    g = torch.empty((d, d), dtype=torch.float64, device=x.device)
    info = torch.empty(2, dtype=torch.int32, device=x.device)
    ws, nb = _pca_ws("pca_gram", n, d, 1, x.device)
    check(_L().scd_pca_gram(handle(), ptr(x), ptr(shift), n, d, ptr(g), ptr(info), ptr(ws), nb, stream_ptr()))
    return g, info


def pca_transform(x, w, shift=None, unit=False):
    """scd_pca_transform: x float32 [n, d], w float32 [m, d], shift float32 [d] or None -> (y float32 [n, m] = fl32(x - shift) w^T, with
    unit each row divided by its float32 L2 norm (a row of norm 0 is zeros); info int32 [2] = rows with a non-finite y, rows of norm 0)."""
    x, shift = _pca_args("pca_transform", x, shift)
    _need_cuda(w)
    n, d = x.shape
    if w.dim() != 2 or w.dtype != torch.float32 or w.shape[1] != d or w.shape[0] < 1:
        raise _lib.ScdError(_lib.SCD_EINVAL, "pca_transform: w float32 [m, d]")
    w, m = w.contiguous(), w.shape[0]
    y = torch.empty((n, m), dtype=torch.float32, device=x.device)
    info = torch.empty(2, dtype=torch.int32, device=x.device)
    ws, nb = _pca_ws("pca_transform", 1, d, m, x.device)
    check(_L().scd_pca_transform(handle(), ptr(x), ptr(shift), ptr(w), n, d, m, int(bool(unit)), ptr(y), ptr(info), ptr(ws), nb, stream_ptr()))
    return y, info


# ----------------------------------------------------------------------------- host solvers
def munkres(cost):
    """linear_assignment (cluster_utils.py:234): int array [n,m] -> sorted pairs [min(n,m),2]."""
    x = np.ascontiguousarray(np.atleast_2d(np.asarray(cost)), dtype=np.int64)
    n, m = x.shape
    out = np.zeros((max(1, min(n, m)), 2), dtype=np.int64)
    npairs = C.c_int(0)
    check(_L().scd_munkres(ptr(x), n, m, ptr(out), C.byref(npairs)))
    res = out[: npairs.value].astype(int)
    res.shape = (-1, 2)
    return res


def munkres_sparse(d, rows, cols, vals):
    """linear_assignment(w.max() - w) for the d x d matrix w with entries w[rows, cols] += vals (assign_name,
    clip_lang_util.py:167-178) without building it: sorted pairs [d,2]."""
    r = np.ascontiguousarray(rows, dtype=np.int32)
    c = np.ascontiguousarray(cols, dtype=np.int32)
    v = np.ascontiguousarray(vals, dtype=np.int64)
    out = np.zeros((max(1, d), 2), dtype=np.int64)
    npairs = C.c_int(0)
    check(_L().scd_munkres_sparse(int(d), int(r.size), ptr(r), ptr(c), ptr(v), ptr(out), C.byref(npairs)))
    res = out[: npairs.value].astype(int)
    res.shape = (-1, 2)
    return res


def transport_solve(cost, size_min, size_max):
    """Size-constrained assignment; raises Exception('There was an issue with the min cost flow input.')
    when infeasible (sskm_constrained.py:349-350)."""
    c = np.ascontiguousarray(cost, dtype=np.int32)
    n, k = c.shape
    labels = np.empty(n, dtype=np.int32)
    total = C.c_int64(0)
    rc = _L().scd_transport_solve(ptr(c), n, k, int(size_min), int(size_max), ptr(labels), C.byref(total))
    if rc == _lib.SCD_EINFEASIBLE:
        raise Exception("There was an issue with the min cost flow input.")
    check(rc)
    return labels, total.value


def transport_solve_batch(costs, size_min, size_max, threads=None, labels_out=None):
    """`costs` int32 [B, n, k] (host, C-contiguous): the B problems on up to `threads` host threads (default: the cores this process
    may use, at most B).  Returns (labels int32 [B, n], totals int64 [B]); raises like transport_solve when a problem is infeasible."""
    c = np.ascontiguousarray(costs, dtype=np.int32)
    b, n, k = c.shape
    labels = labels_out if labels_out is not None else np.empty((b, n), dtype=np.int32)
    assert labels.dtype == np.int32 and labels.flags.c_contiguous and labels.shape == (b, n)
    totals = np.zeros(b, dtype=np.int64)
    if threads is None:
        threads = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    rc = _L().scd_transport_solve_batch(ptr(c), n, k, b, int(size_min), int(size_max), ptr(labels), ptr(totals), int(max(1, threads)))
    if rc == _lib.SCD_EINFEASIBLE:
        raise Exception("There was an issue with the min cost flow input.")
    check(rc)
    return labels, totals


# ----------------------------------------------------------------------------- RCCL exchanges through the C ABI
class Comm:
    """One RCCL communicator on this rank's handle (scd_comm_*): the collectives of the sharded hot path for callers that do
    not go through torch.distributed.  `unique_id` = bytes from Comm.unique_id() on rank 0, shipped to every rank."""

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(_L().scd_comm_unique_id_bytes())
        check(_L().scd_comm_unique_id(buf))
        return buf.raw

    def __init__(self, rank, world, unique_id, device=None):
        _dev[0] = torch.cuda.current_device() if device is None else device
        self.h = handle()
        self.rank, self.world = rank, world
        check(_L().scd_comm_init(self.h, rank, world, C.c_char_p(unique_id)))

    def allreduce_centroids(self, sums, counts, inertia):
        """In-place sum over ranks of the M-step partials; returns (sums, counts int64, inertia)."""
        packed = torch.cat([sums.reshape(-1), counts.to(torch.float64), inertia.reshape(-1)]).contiguous()
        check(_L().scd_allreduce_centroids(self.h, ptr(packed), packed.numel(), _lib.stream_ptr()))
        kd, k = sums.numel(), counts.numel()
        return packed[:kd].reshape(sums.shape), packed[kd:kd + k].round().to(torch.int64), packed[kd + k:]

    def allgather_text(self, wt_shard):
        """wt_shard fp16 [v_shard, d] (equal shards) -> [world * v_shard, d]."""
        wt_shard = wt_shard.to(torch.float16).contiguous()
        out = torch.empty((self.world * wt_shard.shape[0],) + tuple(wt_shard.shape[1:]), dtype=torch.float16, device=wt_shard.device)
        check(_L().scd_allgather_text(self.h, ptr(wt_shard), wt_shard.numel(), ptr(out), _lib.stream_ptr()))
        return out

    def close(self):
        check(_L().scd_comm_destroy(self.h))


# ----------------------------------------------------------------------------- encoders
def gemm_f16(a, w, bias=None, residual=None, act=0, out=None):
    """C = act(a @ w^T + bias) + residual (scd_gemm_f16).  out: the fp16 [m, n] buffer to write - it may be `residual` itself, as in
    the encoder blocks (x = x + proj(...)); a fresh one is allocated when None."""
    _need_cuda(a, w)
    m, k = a.shape
    n = w.shape[0]
    if out is None:
        out = torch.empty((m, n), dtype=torch.float16, device=a.device)
    assert out.dtype == torch.float16 and out.is_contiguous() and out.shape == (m, n) and out.device == a.device
    check(_L().scd_gemm_f16(handle(), ptr(a), ptr(w), ptr(bias), ptr(residual), ptr(out), m, n, k, int(act), stream_ptr()))
    return out


def _f16c(*ts):
    for t in ts:
        assert t.dtype == torch.float16 and t.is_contiguous() and t.is_cuda


def _f32c(*ts):
    for t in ts:
        assert t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda


def gemm_ln_apply_f16(a, wf, biasf, colsum, stats_in, eps, act=0, rs=None, zero_out=None, out=None):
    """The LayerNorm-folded QKV / fc1 GEMM (scd_gemm_ln_apply_f16: scd_gemm_ln_finish, then gemm_w4_kernel LN = 1).  stats_in int64
    [m, 2] fixed-point row sums of a; rs float32 [m, 2] scratch ({rstd, -mean * rstd} afterwards); zero_out int64 [m, 2] is cleared."""
    _need_cuda(a, wf)
    m, k = a.shape
    n = wf.shape[0]
    _f16c(a, wf)
    _f32c(biasf, colsum)
    assert wf.shape == (n, k) and biasf.shape == (n,) and colsum.shape == (n,)
    assert stats_in.dtype == torch.int64 and stats_in.is_contiguous() and stats_in.shape == (m, 2)
    if rs is None:
        rs = torch.empty((m, 2), dtype=torch.float32, device=a.device)
    _f32c(rs)
    assert rs.shape == (m, 2)
    if zero_out is not None:
        assert zero_out.dtype == torch.int64 and zero_out.is_contiguous() and zero_out.shape == (m, 2)
    if out is None:
        out = torch.empty((m, n), dtype=torch.float16, device=a.device)
    _f16c(out)
    assert out.shape == (m, n)
    check(_L().scd_gemm_ln_apply_f16(handle(), ptr(a), ptr(wf), ptr(biasf), ptr(colsum), ptr(stats_in), ptr(rs), ptr(zero_out), ptr(out),
                                     m, n, k, float(eps), int(act), stream_ptr()))
    return out


def gemm_res_stats_f16(a, w, bias, residual, stats_out, out=None, act=0):
    """The proj / fc2 GEMM of a LayerNorm-folded block (scd_gemm_res_stats_f16, gemm_w4_kernel LN = 2): out = a @ w^T + bias + residual
    and stats_out[m] += {sum * 2^24, sum of squares * 2^20} of the stored row m.  out may be `residual` (in place, as the blocks run)."""
    _need_cuda(a, w)
    m, k = a.shape
    n = w.shape[0]
    _f16c(a, w, residual)
    _f32c(bias)
    assert w.shape == (n, k) and bias.shape == (n,) and residual.shape == (m, n)
    assert stats_out.dtype == torch.int64 and stats_out.is_contiguous() and stats_out.shape == (m, 2)
    if out is None:
        out = torch.empty((m, n), dtype=torch.float16, device=a.device)
    _f16c(out)
    assert out.shape == (m, n)
    check(_L().scd_gemm_res_stats_f16(handle(), ptr(a), ptr(w), ptr(bias), ptr(residual), ptr(out), ptr(stats_out), m, n, k, int(act),
                                      stream_ptr()))
    return out


def fold_ln_f16(w, gamma, beta, bias):
    """LayerNorm folded into the Linear that follows it (scd_fold_ln_f16, fold_ln_kernel): returns Wf fp16 [n, k], colsum and biasf
    float32 [n]."""
    _need_cuda(w)
    n, k = w.shape
    _f16c(w)
    _f32c(gamma, beta, bias)
    assert gamma.shape == (k,) and beta.shape == (k,) and bias.shape == (n,)
    wf = torch.empty_like(w)
    colsum = torch.empty(n, dtype=torch.float32, device=w.device)
    biasf = torch.empty(n, dtype=torch.float32, device=w.device)
    check(_L().scd_fold_ln_f16(handle(), ptr(w), ptr(gamma), ptr(beta), ptr(bias), n, k, ptr(wf), ptr(colsum), ptr(biasf), stream_ptr()))
    return wf, colsum, biasf


def gemm_img_f16(pixels, w, m=None):
    """The patch-16 embedding GEMM fed from the image batch (scd_gemm_img_f16, gemm_w4_kernel IMG): pixels fp16 [batch, 3, image, image],
    w fp16 [n, 768] -> fp16 [m, n], m = batch * (image / 16)^2 rounded up to 256 unless given; rows beyond the patches are scratch."""
    _need_cuda(pixels, w)
    _f16c(pixels, w)
    batch, _, image, _ = pixels.shape
    assert pixels.shape == (batch, 3, image, image) and w.shape[1] == 768
    n = w.shape[0]
    if m is None:
        m = (batch * (image // 16) ** 2 + 255) // 256 * 256
    out = torch.empty((m, n), dtype=torch.float16, device=w.device)
    check(_L().scd_gemm_img_f16(handle(), ptr(pixels), ptr(w), ptr(out), int(m), n, batch, image, stream_ptr()))
    return out


def layernorm_f16(x, gamma, beta, eps, row_index=None):
    """The encoders' row LayerNorm (scd_layernorm_f16, layernorm_kernel): out[r] = LN(x[row_index[r]]) (row_index int32 or None)."""
    _need_cuda(x)
    _f16c(x)
    _f32c(gamma, beta)
    width = x.shape[1]
    assert gamma.shape == (width,) and beta.shape == (width,)
    rows = x.shape[0]
    if row_index is not None:
        row_index = row_index.to(device=x.device, dtype=torch.int32).contiguous()
        rows = row_index.shape[0]
    out = torch.empty((rows, width), dtype=torch.float16, device=x.device)
    check(_L().scd_layernorm_f16(handle(), ptr(x), ptr(row_index), rows, width, float(eps), ptr(gamma), ptr(beta), ptr(out), stream_ptr()))
    return out


def attention_f16(qkv, batch, T, heads, causal=False):
    """The encoder blocks' attention (scd_attention_f16): qkv fp16 [batch*T, 3*width] -> out fp16 [batch*T, width]."""
    _need_cuda(qkv)
    width = qkv.shape[1] // 3
    assert qkv.dtype == torch.float16 and qkv.is_contiguous() and qkv.shape == (batch * T, 3 * width)
    out = torch.empty((batch * T, width), dtype=torch.float16, device=qkv.device)
    check(_L().scd_attention_f16(handle(), ptr(qkv), int(batch), int(T), width, int(heads), 1 if causal else 0, ptr(out), stream_ptr()))
    return out


def vit_assemble_f16(patch, patch_bias, cls, pos, registers, batch, T, stats=False):
    """The visual towers' token assembly (scd_vit_assemble_f16): patch fp16 [batch*np, width] (np = T - 1 - nreg), patch_bias float32
    [width] or None, cls float32 [width], pos float32 [1 + np, width], registers float32 [nreg, width] or None -> out fp16 [rows_pad,
    width] with rows_pad = batch*T rounded up to 256 (the rows behind batch*T are zeros); stats=True also returns the rows' int64
    [rows_pad, 2] LayerNorm statistics."""
    _need_cuda(patch)
    _f16c(patch)
    width = patch.shape[1]
    nreg = 0 if registers is None else registers.shape[0]
    np_ = T - 1 - nreg
    _f32c(cls, pos, *[t for t in (patch_bias, registers) if t is not None])
    assert patch.shape == (batch * np_, width) and cls.shape == (width,) and pos.shape == (1 + np_, width)
    assert patch_bias is None or patch_bias.shape == (width,)
    assert registers is None or (nreg > 0 and registers.shape == (nreg, width))
    rows = (batch * T + 255) // 256 * 256
    out = torch.empty((rows, width), dtype=torch.float16, device=patch.device)
    st = torch.empty((rows, 2), dtype=torch.int64, device=patch.device) if stats else None
    check(_L().scd_vit_assemble_f16(handle(), ptr(patch), ptr(patch_bias), ptr(cls), ptr(pos), ptr(registers), nreg, int(batch), int(T),
                                    width, ptr(out), ptr(st), stream_ptr()))
    return (out, st) if stats else out


def attention_single_query_f16(kv, q, qrow, T, heads, causal=False):
    """The last block's one-query attention (scd_attention_single_query_f16): kv fp16 [batch*T, 2*width], q fp16 [batch, width],
    qrow int32 [batch] = b*T + query position (the causal key limit) -> out fp16 [batch, width]."""
    _need_cuda(kv, q)
    batch, width = q.shape
    assert kv.dtype == torch.float16 and q.dtype == torch.float16 and kv.is_contiguous() and q.is_contiguous()
    assert kv.shape == (batch * T, 2 * width)
    if qrow is not None:
        qrow = qrow.to(device=q.device, dtype=torch.int32).contiguous()
        assert qrow.shape == (batch,)
    out = torch.empty((batch, width), dtype=torch.float16, device=q.device)
    check(_L().scd_attention_single_query_f16(handle(), ptr(kv), ptr(q), ptr(qrow), int(batch), int(T), width, int(heads),
                                              1 if causal else 0, ptr(out), stream_ptr()))
    return out


class Encoder:
    """Owns the device weights (kept alive here) and the scd_encoder handle."""

    def __init__(self, desc, weights):
        self.desc = desc
        self.weights = weights              # list of tensors / None in the C order
        _need_cuda(next(w for w in weights if w is not None))
        arr = (C.c_void_p * len(weights))(*[None if w is None else w.data_ptr() for w in weights])
        enc = C.c_void_p()
        d = _lib.EncoderDesc(**desc)
        check(_L().scd_encoder_create(handle(), C.byref(d), arr, len(weights), C.byref(enc)))
        self._enc = enc
        self._ws = None
        self.out_dim = desc["out_dim"] if desc["out_dim"] > 0 else desc["width"]
        self.device = next(w for w in weights if w is not None).device

    def __del__(self):
        try:
            if getattr(self, "_enc", None):
                _L().scd_encoder_destroy(self._enc)
        except Exception:
            pass

    def timing(self, enable):
        """Enable/disable HIP-event timing of the fc1 GEMM launches; returns (ms, launches, flop) collected so far."""
        ms, n, fl = C.c_double(0), C.c_int(0), C.c_double(0)
        check(_L().scd_encoder_timing(self._enc, 1 if enable else 0, C.byref(ms), C.byref(n), C.byref(fl)))
        return ms.value, n.value, fl.value

    def _workspace(self, batch):
        nb = _L().scd_encoder_ws_bytes(self._enc, batch)
        if self._ws is None or self._ws.numel() < nb:
            self._ws = _ws(nb, self.device)
        return self._ws, nb

    def encode_image(self, pixels, normalize=False, out=None):
        """out: an fp16 [B, out_dim] contiguous tensor (e.g. a row slice of the feature matrix) the features are written into."""
        _need_cuda(pixels)
        pixels = pixels.contiguous()
        if pixels.dtype not in (torch.float16, torch.float32):
            pixels = pixels.float()
        b = pixels.shape[0]
        if out is None:
            out = torch.empty((b, self.out_dim), dtype=torch.float16, device=pixels.device)
        assert out.dtype == torch.float16 and out.shape == (b, self.out_dim) and out.is_contiguous() and out.device == pixels.device
        ws, nb = self._workspace(b)
        dt = SCD_F16 if pixels.dtype == torch.float16 else SCD_F32
        check(_L().scd_vit_encode_image(handle(), self._enc, ptr(pixels), dt, b, ptr(out), 1 if normalize else 0, ptr(ws), nb,
                                        stream_ptr()))
        return out

    def encode_text(self, tokens, normalize=False, ctx_len=None):
        """tokens int32 [B, 77] on the device.  ctx_len (> every row's EOT position): compute only the first ctx_len positions
        (scd_clip_encode_text_len: same bits, ctx_len / 77 of the work)."""
        _need_cuda(tokens)
        tokens = tokens.to(torch.int32).contiguous()
        b = tokens.shape[0]
        out = torch.empty((b, self.out_dim), dtype=torch.float16, device=tokens.device)
        ws, nb = self._workspace(b)
        if ctx_len is None or ctx_len >= tokens.shape[1]:
            check(_L().scd_clip_encode_text(handle(), self._enc, ptr(tokens), b, ptr(out), 1 if normalize else 0, ptr(ws), nb,
                                            stream_ptr()))
        else:
            check(_L().scd_clip_encode_text_len(handle(), self._enc, ptr(tokens), b, int(ctx_len), ptr(out), 1 if normalize else 0,
                                                ptr(ws), nb, stream_ptr()))
        return out


# ----------------------------------------------------------------------------- exact t-SNE (docs/design/tsne.md)
def tsne_calibrate(dist2, perplexity):
    """scd_tsne_calibrate: dist2 float64 [n, k] (squared distances of a k-NN graph) -> (p float64 [n, k], every row summing to 1,
    beta float64 [n], info int32 [2] = rows whose entropy cannot reach log(perplexity), rows with a bad distance)."""
    _need_cuda(dist2)
    if dist2.dim() != 2 or dist2.dtype != torch.float64:
        raise _lib.ScdError(_lib.SCD_EINVAL, "tsne_calibrate: dist2 must be float64 [n, k]")
    dist2 = dist2.contiguous()
    n, k = dist2.shape
    p = torch.empty_like(dist2)
    beta = torch.empty(n, dtype=torch.float64, device=dist2.device)
    info = torch.empty(2, dtype=torch.int32, device=dist2.device)
    check(_L().scd_tsne_calibrate(handle(), ptr(dist2), n, k, float(perplexity), ptr(p), ptr(beta), ptr(info), stream_ptr()))
    return p, beta, info


TSNE_EXACT_PAIRS = 1


def tsne_gradient(y, indptr, indices, values, exaggeration=1.0, want_kl=True, ws=None, exact_pairs=False):
    """scd_tsne_gradient: y float32 [n, 2], P in CSR form (indptr int64 [n + 1], indices int32 [nnz], values float64 [nnz]) ->
    (grad float64 [n, 2], z float64 [1], kl float64 [1] or None, info int32 [2] = rows with an out-of-range CSR entry, rows of y that
    are not finite below 2^60), on the device.  exact_pairs: the all-pairs sums in float64 instead of fp32 runs."""
    _need_cuda(y, indptr, indices, values)
    if (y.dim() != 2 or y.shape[1] != 2 or y.dtype != torch.float32 or indptr.dtype != torch.int64 or indices.dtype != torch.int32
            or values.dtype != torch.float64 or indptr.numel() != y.shape[0] + 1 or indices.numel() != values.numel()):
        raise _lib.ScdError(_lib.SCD_EINVAL, "tsne_gradient: y float32 [n, 2], indptr int64 [n + 1], indices int32 [nnz], values float64 [nnz]")
    y, indptr, indices, values = y.contiguous(), indptr.contiguous(), indices.contiguous(), values.contiguous()
    n, nnz = y.shape[0], indices.numel()
    grad = torch.empty((n, 2), dtype=torch.float64, device=y.device)
    z = torch.empty(1, dtype=torch.float64, device=y.device)
    kl = torch.empty(1, dtype=torch.float64, device=y.device) if want_kl else None
    info = torch.empty(2, dtype=torch.int32, device=y.device)
    nb = _L().scd_tsne_gradient_ws_bytes(n, nnz)
    if ws is None or ws.numel() < nb:
        ws = _ws(max(nb, 16), y.device)
    check(_L().scd_tsne_gradient(handle(), ptr(y), ptr(indptr), ptr(indices) if nnz else None, ptr(values) if nnz else None, n, nnz,
                                 float(exaggeration), TSNE_EXACT_PAIRS if exact_pairs else 0, ptr(grad), ptr(z), ptr(kl) if want_kl else None, ptr(info), ptr(ws), nb, stream_ptr()))
    return grad, z, kl, info


def tsne_update(grad, y64, vel, gains, y32, momentum, learning_rate, min_gain=0.01, gg_out=None):
    """scd_tsne_update: one _gradient_descent step on the float64 state (y64, vel, gains: [n, 2], updated in place) and the float32 copy
    y32 the force kernels read; gg_out float64 [n, 2] (optional) receives gains * grad."""
    _need_cuda(grad, y64, vel, gains, y32, gg_out)
    n = y64.shape[0]
    for t in (grad, y64, vel, gains) + (() if gg_out is None else (gg_out,)):
        if t.dtype != torch.float64 or tuple(t.shape) != (n, 2) or not t.is_contiguous():
            raise _lib.ScdError(_lib.SCD_EINVAL, "tsne_update: grad, y64, vel, gains (and gg_out) must be contiguous float64 [n, 2]")
    if y32.dtype != torch.float32 or tuple(y32.shape) != (n, 2) or not y32.is_contiguous():
        raise _lib.ScdError(_lib.SCD_EINVAL, "tsne_update: y32 must be contiguous float32 [n, 2]")
    check(_L().scd_tsne_update(handle(), ptr(grad), ptr(y64), ptr(vel), ptr(gains), ptr(y32), n, float(momentum), float(learning_rate),
                               float(min_gain), None if gg_out is None else ptr(gg_out), stream_ptr()))


# ----------------------------------------------------------------------------- spectral clustering's sparse half (docs/design/spectral.md)
def knn_affinity(idx, cap=None):
    """scd_knn_affinity: idx int32 [n, k] (ops.knn's lists) -> (rowptr int64 [n + 1], col int32 [nnz], val float64 [nnz], inv_sqrt_deg
    float64 [n], nnz), the symmetric normalised affinity S = D^-1/2 (0.5 (C + C^T)) D^-1/2 in CSR form with ascending columns.  cap: the
    capacity handed to the library (default 2 n k, its minimum).  Waits for the stream."""
    _need_cuda(idx)
    if idx.dim() != 2 or idx.dtype != torch.int32:
        raise _lib.ScdError(_lib.SCD_EINVAL, "knn_affinity: idx must be int32 [n, k]")
    idx = idx.contiguous()
    n, k = idx.shape
    cap = 2 * n * k if cap is None else int(cap)
    rowptr = torch.empty(n + 1, dtype=torch.int64, device=idx.device)
    col = torch.empty(max(cap, 1), dtype=torch.int32, device=idx.device)
    val = torch.empty(max(cap, 1), dtype=torch.float64, device=idx.device)
    isd = torch.empty(n, dtype=torch.float64, device=idx.device)
    nb = _L().scd_knn_affinity_ws_bytes(n, k)
    ws = _ws(max(nb, 16), idx.device)
    nnz = C.c_int64(0)
    check(_L().scd_knn_affinity(handle(), ptr(idx), n, k, ptr(rowptr), ptr(col), ptr(val), ptr(isd), cap, C.byref(nnz), ptr(ws), nb, stream_ptr()))
    nnz = int(nnz.value)
    return rowptr, col[:nnz], val[:nnz], isd, nnz


def spmm_f64(rowptr, col, val, x, alpha=1.0, beta=0.0, gamma=0.0, z=None, out=None):
    """scd_spmm_f64: out = alpha (S x) + beta x + gamma z for S in CSR form (rowptr int64 [n + 1], col int32, val float64) and float64
    blocks x, z, out [n, m] with unit column stride (a column slice of a wider buffer is fine: its row stride is the leading dimension).
    m % 8 == 0, row strides multiples of 8; out may alias neither x nor z.  The summation order is fixed (include/scd_hip.h)."""
    _need_cuda(x, rowptr, col, val, z, out)
    n = rowptr.numel() - 1
    if rowptr.dtype != torch.int64 or col.dtype != torch.int32 or val.dtype != torch.float64 or col.numel() != val.numel():
        raise _lib.ScdError(_lib.SCD_EINVAL, "spmm_f64: rowptr int64 [n + 1], col int32 [nnz], val float64 [nnz]")
    if out is None:
        out = torch.empty((n, x.shape[1] if x.dim() == 2 else 0), dtype=torch.float64, device=x.device)
    for name, t in (("x", x), ("z", z), ("out", out)):
        if t is not None and (t.dim() != 2 or t.dtype != torch.float64 or t.shape != x.shape or t.shape[0] != n or t.stride(1) != 1):
            raise _lib.ScdError(_lib.SCD_EINVAL, "spmm_f64: %s must be float64 [n = %d, m] with unit column stride" % (name, n))
    rowptr, col, val = rowptr.contiguous(), col.contiguous(), val.contiguous()
    check(_L().scd_spmm_f64(handle(), ptr(rowptr), ptr(col), ptr(val), n, ptr(x), x.stride(0), x.shape[1], float(alpha), float(beta), float(gamma),
                            None if z is None else ptr(z), 0 if z is None else z.stride(0), ptr(out), out.stride(0), stream_ptr()))
    return out
