"""E-TDNN x-vector extractor and the joint model on top of it (utils/models.py:29-345).

`TDNN`, `XVectorNet_ETDNN_12Layer` and `Etdnn_Xvec_NeuralPlda` keep the reference's constructors, attribute names and
state-dict keys (so its checkpoints and whole-module pickles load), but only the extraction path computes, and it runs as
hand-written HIP (csrc/nplda_xvec.hip through include/nplda_hip.h):

    extract(x)                     (B, 30, T) features -> (B, 512) x-vectors                 (utils/models.py:170-186)
    extract_ragged(frames, lens)   (sum T_u, 30) frames of utterances of different lengths -> (U, 512)
    extract_windows(frames, wins)  (R, 30) frames and (W, 2) [begin, end) row windows -> (W, 512): sliding-window x-vectors
                                   from one dense pass, bit for bit extract_ragged on the cut-outs (design/k23)
    extract_from_scp(feats_scp)    a Kaldi feature scp (+ VAD) -> keys, (U, 512): features.py's front end, then extract_ragged
    Etdnn_Xvec_NeuralPlda.forward  extract both sides, then the existing HIP NPLDA head       (utils/models.py:251-268)

Batch norm runs with its running statistics only (the reference's `train1()` puts the tdnn batch norms in eval mode).
By default there is no backward through the extractor: with grad mode on, a parameter of the extractor that requires
grad is an error, and a frozen extractor (`xvector_extractor.requires_grad_(False)`) trains the head through the head's
own HIP backward.

`XVectorNet_ETDNN_12Layer.enable_backward()` (or `Etdnn_Xvec_NeuralPlda.train1(finetune_extractor=True)`) turns on the
end-to-end path: with grad mode on and an extractor parameter that requires grad, `extract` / `extract_ragged` run a
training forward (csrc/nplda_xvec_bwd.hip: the same GEMMs, so the same x-vectors bit for bit) that keeps every layer's
activations and ReLU masks, about 30 KB per frame (`nplda_xvec_train_saved_bytes`: 30.7 KB per frame plus 12 KB per
utterance) held until backward, and the backward returns the gradients of the 22 tdnn1..tdnn10 / lin11 weights and biases
through HIP kernels (bn11, bn12, lin12 and finlin keep grad None, as in the reference).  The training path does not
chunk a batch: one call per side.  There is no dL/dMFCC (an input that requires grad is an error).  The classifier path
(`forward`, `prestatspool`, `postpooling`) is not provided.

`XVectorNet_ETDNN_12Layer.enable_batch_stats()` opts in to batch-statistics batch norm (design/k27_xvec_batch_stats.md):
with it on and all ten tdnn batch norms in training mode (a plain `model.train()`), `extract` / `extract_ragged`
normalise every tdnn layer by the mean and biased variance of the call's own valid frames and update the running
statistics as torch does (csrc/nplda_xvec_bn.hip), forward-only or, with `enable_backward()` under grad mode, through an
autograd Function whose backward includes the batch-norm backward.  One call covers the whole batch.  With the switch
off, or all ten in eval mode, everything above holds unchanged.
"""
import ctypes
import os
import pickle

import numpy as np
import torch
import torch.nn as nn

from . import _lib, features, kaldi_format
from .models import NeuralPlda, _compute_device

__all__ = ["TDNN", "XVectorNet_ETDNN_12Layer", "Etdnn_Xvec_NeuralPlda", "LAYERS", "CONTEXT", "flops_per_frame",
           "plan_windows", "WindowChunk"]

# (Din, Dout, context, dilation) of tdnn1..tdnn10 (utils/models.py:104-123)
LAYERS = ((30, 512, 5, 1), (512, 512, 1, 1), (512, 512, 3, 2), (512, 512, 1, 1), (512, 512, 3, 3), (512, 512, 1, 1),
          (512, 512, 3, 4), (512, 512, 1, 1), (512, 512, 1, 1), (512, 1500, 1, 1))
CONTEXT = sum(d * (c - 1) for _, _, c, d in LAYERS)  # 22 frames lost per utterance
FEAT, XVEC_DIM, POOL_DIM = 30, 512, 1500
LAYOUT_ROWS, LAYOUT_BCT = 0, 1  # include/nplda_hip.h NPLDA_XVEC_LAYOUT_*
POOL_STD, POOL_VAR = 0, 1       # NPLDA_XVEC_POOL_*
MAX_WORKSPACE_BYTES = 1 << 30   # per extraction call; larger batches are split by utterance
MAX_BATCH_STATS_BYTES = 1 << 34  # `saved` of one batch-statistics call (about 31 KB per frame); larger batches raise


def flops_per_frame():
    """Algorithmic FLOP per frame of tdnn1..tdnn10 (2 K N each) and per utterance of lin11."""
    frame = sum(2 * c * din * dout for din, dout, c, _ in LAYERS)
    return frame, 2 * 2 * POOL_DIM * XVEC_DIM


# nplda_xvec_workspace_bytes restated (csrc/nplda_xvec.hip ws_layout) so that a batch is split without a call per utterance
def _ws_bytes(R, U):
    a = lambda b: (b + 255) // 256 * 256  # noqa: E731
    rows = (R + 127) // 128 * 128 + 16
    urows = (U + 127) // 128 * 128
    oA = a(rows * 32 * 4)
    oB = a(oA + rows * 512 * 4)
    oP = a(oB + rows * 1504 * 4)
    return a(oP + urows * 3008 * 4)


def _chunks(lengths, limit):
    """[(u0, u1)] runs of whole utterances whose workspace stays within `limit` bytes (one utterance at least)."""
    out, u0, R = [], 0, 0
    for u, T in enumerate(lengths):
        if u > u0 and _ws_bytes(R + T, u + 1 - u0) > limit:
            out.append((u0, u))
            u0, R = u, 0
        R += T
    if u0 < len(lengths):
        out.append((u0, len(lengths)))
    return out


class WindowChunk:
    """One extraction call of plan_windows: `windows` (indices into the caller's table, in order of begin), `intervals`
    ([(b, e)] disjoint ascending runs of the caller's rows: the union of the windows' rows, laid end to end as the call's
    input), `begin` / `end` (int64 rows of each window inside that input) and `rows` (input rows)."""

    def __init__(self, windows, intervals, begin, end):
        self.windows, self.intervals, self.begin, self.end = windows, intervals, begin, end
        self.rows = int(sum(e - b for b, e in intervals))


def plan_windows(windows, limit):
    """Split a (W, 2) table of [begin, end) row windows into extraction calls whose workspace stays within `limit` bytes
    (a window that does not fit on its own still runs alone) -> [WindowChunk].  The windows are taken in order of begin.
    A call's input is the union of its windows' rows: rows that no window covers are never run through the layers, and
    a cut between two calls recomputes only the rows that windows on both sides of it cover.  A window pools only rows
    whose context lies inside its own rows, so neither the laying end to end nor a cut changes a bit of the result."""
    win = np.asarray(windows, dtype=np.int64).reshape(-1, 2)
    order = np.lexsort((win[:, 1], win[:, 0]))
    B, E = win[order, 0], win[order, 1]
    W, s, chunks = order.size, 0, []
    while s < W:
        K = 64  # windows looked at: grown until the cut (or the table's end) lies inside
        while True:
            hi = min(s + K, W)
            b, e = B[s:hi], E[s:hi]
            top = np.maximum.accumulate(e)
            prev = np.concatenate([b[:1], top[:-1]])  # where the union of the windows before this one ends
            new = b > prev                            # a gap in front: the window opens an interval
            new[0] = True
            rows = np.cumsum(np.where(new, e - b, np.maximum(e - prev, 0)))
            over = _ws_bytes(rows, np.arange(1, hi - s + 1)) > limit
            over[0] = False
            if over.any():
                n = int(np.argmax(over))
                break
            if hi == W:
                n = hi - s
                break
            K *= 4
        first = np.flatnonzero(new[:n])
        last = np.concatenate([first[1:], [n]]) - 1   # the last window of each interval
        iv = np.cumsum(new[:n]) - 1                   # each window's interval
        iv_end, iv_rows = top[last][iv], rows[last][iv]
        chunks.append(WindowChunk(order[s:s + n], list(zip(b[first].tolist(), top[last].tolist())),
                                  iv_rows - (iv_end - b[:n]), iv_rows - (iv_end - e[:n])))
        s += n
    return chunks


def _pool_kind(fn):
    if fn is torch.std:
        return POOL_STD
    if fn is torch.var:
        return POOL_VAR
    raise ValueError(f"pooling_function {fn!r}: the HIP extractor implements torch.std and torch.var")


class TDNN(nn.Module):
    """utils/models.py:29-96: same constructor, attributes and parameters.  It computes only inside
    XVectorNet_ETDNN_12Layer.extract, where the ten layers run as one chain of HIP GEMMs."""

    def __init__(self, input_dim=23, output_dim=512, context_size=5, stride=1, dilation=1, batch_norm=True):
        super(TDNN, self).__init__()
        self.context_size = context_size
        self.stride = stride
        self.input_dim = input_dim
        self.output_dim = output_dim
        self.dilation = dilation
        self.padlen = int(dilation * (context_size - 1) / 2)
        self.kernel = nn.Linear(input_dim * context_size, output_dim)
        self.nonlinearity = nn.ReLU()
        self.batch_norm = batch_norm
        if batch_norm:
            self.bn = nn.BatchNorm1d(output_dim, affine=False)

    def forward(self, x):
        raise NotImplementedError("a single TDNN layer runs only inside XVectorNet_ETDNN_12Layer.extract (HIP)")


class XVectorNet_ETDNN_12Layer(nn.Module):
    """utils/models.py:98-214: the 12-layer E-TDNN x-vector network.  `extract` / `extract_ragged` run on HIP."""

    backward_enabled = False  # class attribute: pickles written before the switch existed load with it off
    batch_stats_enabled = False  # likewise
    _bn_alloc = None  # tests: a callable (bytes, device, "saved" | "ws") -> uint8 tensor for the batch-statistics buffers

    def __init__(self, noclasses=13539, pooling_function=torch.std):
        super(XVectorNet_ETDNN_12Layer, self).__init__()
        for i, (din, dout, c, d) in enumerate(LAYERS, 1):
            setattr(self, f"tdnn{i}", TDNN(input_dim=din, output_dim=dout, context_size=c, dilation=d))
        self.pooling_function = pooling_function
        self.lin11 = nn.Linear(3000, 512)
        self.bn11 = nn.BatchNorm1d(num_features=512, affine=False)
        self.bn12 = nn.BatchNorm1d(num_features=512, affine=False)
        self.lin12 = nn.Linear(512, 512)
        self.finlin = nn.Linear(512, noclasses)
        self.smax = nn.Softmax(dim=1)
        self._xvec_cache = {}

    def __setstate__(self, state):
        super(XVectorNet_ETDNN_12Layer, self).__setstate__(state)
        self.__dict__["_xvec_cache"] = {}

    def __getstate__(self):
        state = self.__dict__.copy()
        state["_xvec_cache"] = {}  # device buffers do not belong in a model file
        return state

    def tdnns(self):
        return [getattr(self, f"tdnn{i}") for i in range(1, 11)]

    def invalidate_packed(self):
        """Drop the packed weight image (needed only after writes that bypass the version counters, e.g. a foreign kernel;
        `.data` writes of LoadFromKaldi, in-place ops and optimiser steps are noticed)."""
        self.__dict__["_xvec_cache"] = {}

    def train(self, mode=True):
        self.invalidate_packed()
        return super(XVectorNet_ETDNN_12Layer, self).train(mode)

    def enable_backward(self, flag=True):
        """Opt in to backpropagation through `extract` / `extract_ragged` (a plain attribute, not state-dict content)."""
        self.backward_enabled = bool(flag)
        return self

    def enable_batch_stats(self, flag=True):
        """Opt in to batch-statistics batch norm: with the switch on and all ten tdnn<i>.bn in training mode, `extract` /
        `extract_ragged` normalise by the statistics of the call's frames and update the running statistics (a plain
        attribute, not state-dict content).  With all ten in eval mode the switch changes nothing."""
        self.batch_stats_enabled = bool(flag)
        return self

    def forward(self, x):
        raise NotImplementedError("the classifier path (utils/models.py:158-168) is not provided: use extract()")

    # -- packed weights -------------------------------------------------------------------------
    def _sources(self):
        ts = self.tdnns()
        return ([t.kernel.weight for t in ts] + [self.lin11.weight], [t.kernel.bias for t in ts] + [self.lin11.bias],
                [t.bn.running_mean for t in ts], [t.bn.running_var for t in ts], [float(t.bn.eps) for t in ts])

    def _check_mode(self, x):
        for i, t in enumerate(self.tdnns(), 1):
            bn = t.bn
            if bn.training or bn.running_mean is None or bn.running_var is None:
                raise RuntimeError(f"tdnn{i}.bn is in training mode (batch statistics): the HIP extractor implements "
                                   "running-statistics batch norm only; call .eval() (or Etdnn_Xvec_NeuralPlda.train1())")
        if torch.is_grad_enabled():
            if any(p.requires_grad for p in self.parameters()):
                raise RuntimeError("no backward through the x-vector extractor: freeze it with "
                                   "xvector_extractor.requires_grad_(False) or extract under torch.no_grad()")
            if x.requires_grad:
                raise RuntimeError("no backward through the x-vector extractor: its input must not require grad")

    def _packed(self, dev):
        """The fragment-ordered weight image on `dev`, rebuilt when any source tensor is replaced or changes version.  The
        cache holds the source tensors themselves, so a freed parameter whose address is reused cannot hit."""
        W, b, m, v, eps = self._sources()
        srcs = W + b + m + v
        cache = self.__dict__.setdefault("_xvec_cache", {})
        key = (dev, tuple(t._version for t in srcs), tuple(eps))
        held = cache.get("srcs")
        if (cache.get("key") == key and held is not None and len(held) == len(srcs)
                and all(a is b_ for a, b_ in zip(held, srcs))):
            return cache["buf"]
        lib = _lib.load()
        with _lib.on_device(dev):
            dsrc = [t.detach().to(dev, torch.float32).contiguous() for t in srcs]
            n = lib.nplda_xvec_packed_bytes()
            buf = torch.empty(n, dtype=torch.uint8, device=dev)
            ptrs = [(ctypes.c_void_p * len(a))(*[t.data_ptr() for t in a])
                    for a in (dsrc[:11], dsrc[11:22], dsrc[22:32], dsrc[32:42])]
            e = (ctypes.c_float * 10)(*eps)
            # (the device copies die with this frame: the caching allocator reuses them in stream order, after the pack)
            _lib.check(lib.nplda_xvec_pack_f32(*ptrs, e, buf.data_ptr(), n, _lib.current_stream(dev)),
                       "nplda_xvec_pack_f32")
        cache.clear()
        cache.update(key=key, srcs=list(srcs), buf=buf)
        return buf

    def _packed_t(self, dev):
        """The transposed weight image of the data gradient, cached next to `_packed(dev)` under the same key."""
        self._packed(dev)
        cache = self.__dict__["_xvec_cache"]
        if cache.get("buf_t") is None:
            lib = _lib.load()
            with _lib.on_device(dev):
                W = [t.detach().to(dev, torch.float32).contiguous() for t in self._sources()[0]]
                n = lib.nplda_xvec_packed_t_bytes()
                buf = torch.empty(n, dtype=torch.uint8, device=dev)
                ptrs = (ctypes.c_void_p * len(W))(*[t.data_ptr() for t in W])
                _lib.check(lib.nplda_xvec_pack_t_f32(ptrs, buf.data_ptr(), n, _lib.current_stream(dev)),
                           "nplda_xvec_pack_t_f32")
            cache["buf_t"] = buf
        return cache["buf_t"]

    def _grad_params(self):
        """tdnn1.W, tdnn1.b, ..., tdnn10.b, lin11.W, lin11.b: the order of nplda_xvec_backward_f32's flat gradient."""
        out = []
        for m in [t.kernel for t in self.tdnns()] + [self.lin11]:
            out += [m.weight, m.bias]
        return out

    def _wants_backward(self, x):
        """True when extraction must record for autograd (the switch is on, grad mode is on and an extractor parameter
        requires grad); raises for what the training path does not provide."""
        if not (self.backward_enabled and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())):
            return False
        for i, t in enumerate(self.tdnns(), 1):
            bn = t.bn
            if bn.training or bn.running_mean is None or bn.running_var is None:
                raise RuntimeError(f"tdnn{i}.bn is in training mode (batch statistics): the HIP extractor implements "
                                   "running-statistics batch norm only; call .eval() (or Etdnn_Xvec_NeuralPlda.train1())")
        if x.requires_grad:
            raise RuntimeError("no backward through the x-vector extractor: its input must not require grad")
        return True

    def _wants_batch_stats(self):
        """True when the batch-statistics switch is on and all ten tdnn batch norms are in training mode; False when the
        switch is off or all ten are in eval mode (the running-statistics paths, unchanged); raises for anything else."""
        if not self.batch_stats_enabled:
            return False
        bns = [t.bn for t in self.tdnns()]
        flags = [bool(bn.training) for bn in bns]
        if not any(flags):
            return False
        if not all(flags):
            on = [f"tdnn{i}" for i, f in enumerate(flags, 1) if f]
            raise RuntimeError(f"mixed batch-norm modes: {', '.join(on)} in training mode and the rest in eval mode; "
                               "batch statistics need all ten tdnn batch norms in training mode (model.train()), "
                               "running statistics all ten in eval mode (.eval() or Etdnn_Xvec_NeuralPlda.train1())")
        for i, bn in enumerate(bns, 1):
            if bn.running_mean is None or bn.running_var is None:
                raise RuntimeError(f"tdnn{i}.bn has no running statistics (track_running_stats=False): not implemented")
            if bn.momentum is None:
                raise RuntimeError(f"tdnn{i}.bn.momentum is None (cumulative moving average): not implemented, "
                                   "set a momentum")
        return True

    def _check_batch_stats(self, x, lengths):
        """The host-side checks of the batch-statistics path (before any device is touched) -> whether to record for
        autograd."""
        grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if grad and not self.backward_enabled:
            raise RuntimeError("no backward through the x-vector extractor: freeze it with "
                               "xvector_extractor.requires_grad_(False), extract under torch.no_grad() or call "
                               "enable_backward()")
        if torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError("no backward through the x-vector extractor: its input must not require grad")
        U, R = len(lengths), int(sum(lengths))
        if U > 0 and R - U * CONTEXT < 2:
            raise ValueError(f"Expected more than 1 value per channel when training: {U} utterance(s) of {R} frames leave "
                             f"{R - U * CONTEXT} frame(s) after the context of {CONTEXT}")
        return grad

    def _extract_batch_stats(self, X, layout, lengths, dev, workspace_bytes, grad):
        """The batch-statistics path of extract / extract_ragged: X on `dev`, float32 contiguous."""
        U, R = len(lengths), int(sum(lengths))
        if U == 0:
            return torch.empty((0, XVEC_DIM), dtype=torch.float32, device=dev)
        n = _lib.load().nplda_xvec_train_bn_saved_bytes(R, U)
        limit = MAX_BATCH_STATS_BYTES if workspace_bytes is None else int(workspace_bytes)
        if n > limit:
            raise RuntimeError(f"batch-statistics extraction of {R} frames needs {n} bytes of saved activations, above "
                               f"the limit of {limit} bytes; the statistics span the batch, so it is not split")
        if grad:
            return _ExtractBnFn.apply(self, X, layout, lengths, dev, *self._grad_params())
        return _bn_forward(self, X, layout, lengths, dev)[0]

    # -- extraction ------------------------------------------------------------------------------
    def _run(self, x, layout, lengths, dev, workspace_bytes):
        """x on `dev`, float32 contiguous: (sum T, 30) for LAYOUT_ROWS, (U, 30, T) for LAYOUT_BCT."""
        U = len(lengths)
        out = torch.empty((U, XVEC_DIM), dtype=torch.float32, device=dev)
        if U == 0:
            return out
        packed = self._packed(dev)
        kind = _pool_kind(self.pooling_function)
        lib = _lib.load()
        limit = MAX_WORKSPACE_BYTES if workspace_bytes is None else int(workspace_bytes)
        starts = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        with _lib.on_device(dev):
            st = _lib.current_stream(dev)
            for u0, u1 in _chunks(lengths, limit):
                f0, f1 = int(starts[u0]), int(starts[u1])
                offs = torch.from_numpy(starts[u0:u1 + 1] - f0).to(dev)
                ws_n = lib.nplda_xvec_workspace_bytes(f1 - f0, u1 - u0)
                ws = torch.empty(ws_n, dtype=torch.uint8, device=dev)
                src = x[f0:f1] if layout == LAYOUT_ROWS else x[u0:u1]
                _lib.check(lib.nplda_xvec_extract_f32(src.data_ptr(), layout, FEAT, offs.data_ptr(), u1 - u0, f1 - f0, kind,
                                                      packed.data_ptr(), out[u0:u1].data_ptr(), XVEC_DIM, ws.data_ptr(),
                                                      ws_n, st), "nplda_xvec_extract_f32")
        return out

    def extract(self, x, workspace_bytes=None):
        """utils/models.py:170-186: x (B, 30, T) -> (B, 512) x-vectors = lin11([mean | std] of tdnn10 ... tdnn1 (x^T)),
        on the HIP device (CPU input is staged through it and the result returned on the input's device)."""
        if x.dim() != 3 or x.shape[1] != FEAT:
            raise ValueError(f"extract expects (B, {FEAT}, T) features, got {tuple(x.shape)}")
        bstats = self._wants_batch_stats()
        grad = False if bstats else self._wants_backward(x)
        if not (grad or bstats):
            self._check_mode(x)
        B, _, T = x.shape
        if B > 0 and T <= CONTEXT:
            raise ValueError(f"T = {T} frames is shorter than the extractor's context ({CONTEXT + 1} frames at least)")
        if bstats:
            grad = self._check_batch_stats(x, [T] * B)
        dev = _compute_device(x, self.lin11.weight)
        X = x.detach().to(dev, torch.float32).contiguous()
        if bstats:
            out = self._extract_batch_stats(X, LAYOUT_BCT, [T] * B, dev, workspace_bytes, grad)
        elif grad:
            out = _ExtractFn.apply(self, X, LAYOUT_BCT, [T] * B, dev, *self._grad_params())
        else:
            out = self._run(X, LAYOUT_BCT, [T] * B, dev, workspace_bytes)
        return out if out.device == x.device else out.to(x.device)

    def extract_ragged(self, frames, lengths, workspace_bytes=None):
        """x-vectors of utterances of different lengths: frames (sum T_u, 30) row-major, utterance u being the next
        lengths[u] rows; -> (len(lengths), 512).  Same values as extract() on each utterance alone, bit for bit."""
        if frames.dim() != 2 or frames.shape[1] != FEAT:
            raise ValueError(f"extract_ragged expects (frames, {FEAT}) rows, got {tuple(frames.shape)}")
        lengths = [int(T) for T in (lengths.tolist() if isinstance(lengths, (torch.Tensor, np.ndarray)) else lengths)]
        if sum(lengths) != frames.shape[0]:
            raise ValueError(f"lengths sum to {sum(lengths)}, frames has {frames.shape[0]} rows")
        short = [T for T in lengths if T <= CONTEXT]
        if short:
            raise ValueError(f"an utterance of {short[0]} frames is shorter than the extractor's context "
                             f"({CONTEXT + 1} frames at least; the reference's unfold raises)")
        bstats = self._wants_batch_stats()
        grad = False if bstats else self._wants_backward(frames)
        if not (grad or bstats):
            self._check_mode(frames)
        if bstats:
            grad = self._check_batch_stats(frames, lengths)
        dev = _compute_device(frames, self.lin11.weight)
        X = frames.detach().to(dev, torch.float32).contiguous()
        if bstats:
            out = self._extract_batch_stats(X, LAYOUT_ROWS, lengths, dev, workspace_bytes, grad)
        elif grad:
            out = _ExtractFn.apply(self, X, LAYOUT_ROWS, lengths, dev, *self._grad_params())
        else:
            out = self._run(X, LAYOUT_ROWS, lengths, dev, workspace_bytes)
        return out if out.device == frames.device else out.to(frames.device)

    def extract_windows(self, frames, windows, workspace_bytes=None):
        """Sliding-window x-vectors: frames (R, 30) rows, windows (W, 2) integer [begin, end) rows (array, tensor or list;
        they may overlap, repeat and come in any order; the rows of a window are consecutive frames of one recording) ->
        (W, 512) in the caller's window order.  Row w is bit for bit extract_ragged(frames[begin:end], [end - begin]), but
        every covered frame runs through tdnn1..tdnn10 once per call, not once per window (nplda_xvec_extract_windows_f32).
        A table whose workspace exceeds workspace_bytes (default MAX_WORKSPACE_BYTES) is worked through in order of begin
        by plan_windows, which does not change a bit.  Inference only."""
        if frames.dim() != 2 or frames.shape[1] != FEAT:
            raise ValueError(f"extract_windows expects (frames, {FEAT}) rows, got {tuple(frames.shape)}")
        win = np.asarray(windows.cpu() if isinstance(windows, torch.Tensor) else windows)
        if win.size == 0:
            win = np.zeros((0, 2), np.int64)
        if win.ndim != 2 or win.shape[1] != 2 or win.dtype.kind not in "iu":
            raise ValueError(f"windows must be (W, 2) integer [begin, end) rows, got {win.dtype} {win.shape}")
        win = win.astype(np.int64)
        R, W = int(frames.shape[0]), int(win.shape[0])
        bad = np.flatnonzero((win[:, 0] < 0) | (win[:, 1] > R))
        if bad.size:
            w = int(bad[0])
            raise ValueError(f"window {w} = [{win[w, 0]}, {win[w, 1]}) lies outside the {R} rows of frames")
        short = np.flatnonzero(win[:, 1] - win[:, 0] <= CONTEXT)
        if short.size:
            w = int(short[0])
            raise ValueError(f"window {w} = [{win[w, 0]}, {win[w, 1]}) has {win[w, 1] - win[w, 0]} frames, shorter than the "
                             f"extractor's context ({CONTEXT + 1} frames at least)")
        self._check_mode(frames)  # (no training path here: a trainable extractor under grad mode is an error)
        dev = _compute_device(frames, self.lin11.weight)
        out = torch.empty((W, XVEC_DIM), dtype=torch.float32, device=dev)
        if W:
            X = frames.detach().to(dev, torch.float32).contiguous()
            packed = self._packed(dev)
            kind = _pool_kind(self.pooling_function)
            lib = _lib.load()
            limit = MAX_WORKSPACE_BYTES if workspace_bytes is None else int(workspace_bytes)
            with _lib.on_device(dev):
                st = _lib.current_stream(dev)
                w0 = 0
                order = []
                for ch in plan_windows(win, limit):
                    n = len(ch.windows)
                    src = (X[ch.intervals[0][0]:ch.intervals[0][1]] if len(ch.intervals) == 1
                           else torch.cat([X[b:e] for b, e in ch.intervals]))
                    tab = torch.from_numpy(np.stack([ch.begin, ch.end])).to(dev)
                    ws_n = lib.nplda_xvec_windows_workspace_bytes(ch.rows, n)
                    ws = torch.empty(ws_n, dtype=torch.uint8, device=dev)
                    _lib.check(lib.nplda_xvec_extract_windows_f32(src.data_ptr(), FEAT, ch.rows, tab[0].data_ptr(),
                                                                  tab[1].data_ptr(), n, kind, packed.data_ptr(),
                                                                  out[w0:w0 + n].data_ptr(), XVEC_DIM, ws.data_ptr(), ws_n,
                                                                  st), "nplda_xvec_extract_windows_f32")
                    order.append(ch.windows)
                    w0 += n
                order = np.concatenate(order)
                if not np.array_equal(order, np.arange(W)):  # rows came out in order of begin: back to the caller's
                    inv = np.empty(W, np.int64)
                    inv[order] = np.arange(W)
                    out = out.index_select(0, torch.from_numpy(inv).to(dev))
        return out if out.device == frames.device else out.to(frames.device)

    def extract_from_scp(self, feats_scp, vad=features.VadOptions(), cmn_window=300, min_frames=25, utts_per_call=2048,
                         device=None):
        """The recipe's `apply-cmvn-sliding | select-voiced-frames | nnet3-xvector-compute` over a Kaldi feats.scp (FM, DM,
        CM, CM2, CM3 entries): -> (keys, (len(keys), 512) x-vectors on the device, dropped).  vad: features.VadOptions
        (energy VAD on the device), a {key: 0/1 vector} dict, the path of a vad.scp, or None to keep every frame.
        Utterances with fewer than min_frames (>= 24, the extractor's context plus two) voiced frames are not extracted:
        they come back in `dropped` as (key, voiced frames).  The scp is worked through utts_per_call lines at a time, so
        that the host payload, its device copy and the workspaces stay bounded; the pieces do not change the result (bit
        for bit).  Inference only (runs under torch.no_grad())."""
        if int(min_frames) < CONTEXT + 2:
            raise ValueError(f"min_frames = {min_frames}: the extractor needs {CONTEXT + 2} frames at least")
        if int(utts_per_call) < 1:
            raise ValueError("utts_per_call must be positive")
        dev = _compute_device(self.lin11.weight) if device is None else torch.device(device)
        vad_index, maps = None, {}
        if isinstance(vad, (str, os.PathLike)):
            vad_index = dict(kaldi_format.read_scp(vad))
        entries = kaldi_format.read_scp(feats_scp)
        keys, dropped, parts = [], [], []
        for lo in range(0, len(entries), int(utts_per_call)):
            piece = entries[lo:lo + int(utts_per_call)]
            feats = kaldi_format.load_feature_scp(feats_scp, entries=piece, cols=FEAT)
            v = vad
            if vad_index is not None:
                v = {}
                for k, _ in piece:
                    if k not in vad_index:
                        raise KeyError(f"{k}: not in {vad}")
                    f, off = kaldi_format._split_rx(vad_index[k])
                    if f not in maps:
                        maps[f] = np.memmap(kaldi_format._scp_file(f, vad), dtype=np.uint8, mode="r")
                    v[k] = kaldi_format._vec_at(maps[f], off or 0)
            prep = features.prepare_features(feats, vad=v, cmn_window=cmn_window, min_frames=min_frames, device=dev)
            keys += prep.keys
            dropped += prep.dropped
            if prep.keys:
                with torch.no_grad():
                    parts.append(self.extract_ragged(prep.frames, prep.lengths))
        if not parts:
            return keys, torch.empty((0, XVEC_DIM), dtype=torch.float32, device=dev), dropped
        return keys, (parts[0] if len(parts) == 1 else torch.cat(parts)), dropped

    def extract_from_wav_scp(self, wav_scp, mfcc=None, vad=features.VadOptions(), cmn_window=300, min_frames=25,
                             utts_per_call=256, device=None, channel=0, augmenter=None, resample=False):
        """The whole front of the recipe over a Kaldi wav.scp of 16-bit PCM files: `compute-mfcc-feats --dither=0 |
        compute-vad-energy | apply-cmvn-sliding | select-voiced-frames | nnet3-xvector-compute`, nothing leaving the
        device in between -> (keys, (len(keys), 512) x-vectors on the device, dropped), as extract_from_scp.  mfcc: an
        mfcc.MfccOptions with num_ceps == 30 (default: 16 kHz, 30 mel bins, 30 cepstra, 20 - 7600 Hz, snip_edges=false).
        vad: features.VadOptions, a {key: 0/1 vector} dict, or None.  The scp is worked through utts_per_call lines at a
        time; the pieces do not change the result (bit for bit).  augmenter: an augment.Augmenter; each piece is then
        augmented on the device (reverberation, noise, music, babble as it draws them for the piece's utterances, in scp
        order) before its MFCCs; None leaves the audio as it is.  resample: files at another rate than
        mfcc.sample_frequency are resampled on the device (neuralplda_amd.resample) instead of being an error.  Inference
        only."""
        from . import mfcc as _mfcc
        if mfcc is None:
            mfcc = _mfcc.MfccOptions(sample_frequency=16000, num_mel_bins=30, num_ceps=30, low_freq=20, high_freq=7600,
                                     snip_edges=False)
        if mfcc.num_ceps != FEAT:
            raise ValueError(f"MfccOptions.num_ceps = {mfcc.num_ceps}, the extractor takes {FEAT}")
        if int(min_frames) < CONTEXT + 2:
            raise ValueError(f"min_frames = {min_frames}: the extractor needs {CONTEXT + 2} frames at least")
        if int(utts_per_call) < 1:
            raise ValueError("utts_per_call must be positive")
        if isinstance(vad, (str, os.PathLike)):
            raise ValueError("extract_from_wav_scp: vad is VadOptions, a dict of decisions or None (a vad.scp belongs to "
                             "the feats.scp it was computed from)")
        dev = _compute_device(self.lin11.weight) if device is None else torch.device(device)
        entries = kaldi_format.read_scp(wav_scp)
        keys, dropped, parts = [], [], []
        for lo in range(0, len(entries), int(utts_per_call)):
            piece = entries[lo:lo + int(utts_per_call)]
            if resample:
                pkeys, offsets, samples, rates = kaldi_format.load_wav_scp(wav_scp, entries=piece, channel=channel,
                                                                           return_rates=True)
                if (rates != int(mfcc.sample_frequency)).any():
                    from . import resample as _resample
                    samples, offsets, _ = _resample.resample(samples, offsets, rates, int(mfcc.sample_frequency), device=dev)
            else:
                pkeys, offsets, samples = kaldi_format.load_wav_scp(wav_scp, entries=piece,
                                                                    sample_frequency=mfcc.sample_frequency, channel=channel)
            if augmenter is not None:
                samples, offsets, _ = augmenter(samples, offsets, device=dev)
            frames, lengths = _mfcc.compute_mfcc(samples, offsets, mfcc, dev)
            prep = features.prepare_frames(pkeys, frames, lengths, vad, cmn_window, min_frames)
            keys += prep.keys
            dropped += prep.dropped
            if prep.keys:
                with torch.no_grad():
                    parts.append(self.extract_ragged(prep.frames, prep.lengths))
        if not parts:
            return keys, torch.empty((0, XVEC_DIM), dtype=torch.float32, device=dev), dropped
        return keys, (parts[0] if len(parts) == 1 else torch.cat(parts)), dropped

    # -- Kaldi -----------------------------------------------------------------------------------
    def LoadFromKaldi(self, weightspath):
        """utils/models.py:188-214: a pickle of {component: {'params' | 'bias' | 'stats-mean' | 'stats-var': ndarray}}."""
        with open(weightspath, 'rb') as f:
            kw = pickle.load(f)
        sd = self.state_dict()

        def put(name, arr):
            sd[name].data.copy_(torch.from_numpy(np.asarray(arr)).float())

        for i in range(1, 11):
            put(f'tdnn{i}.kernel.weight', kw[f'tdnn{i}.affine']['params'])
            put(f'tdnn{i}.kernel.bias', kw[f'tdnn{i}.affine']['bias'])
            put(f'tdnn{i}.bn.running_mean', kw[f'tdnn{i}.batchnorm']['stats-mean'])
            put(f'tdnn{i}.bn.running_var', kw[f'tdnn{i}.batchnorm']['stats-var'])
        put('lin11.weight', kw['tdnn11.affine']['params'])
        put('lin11.bias', kw['tdnn11.affine']['bias'])
        put('bn11.running_mean', kw['tdnn11.batchnorm']['stats-mean'])
        put('bn11.running_var', kw['tdnn11.batchnorm']['stats-var'])
        put('lin12.weight', kw['tdnn12.affine']['params'])
        put('lin12.bias', kw['tdnn12.affine']['bias'])
        put('bn12.running_mean', kw['tdnn12.batchnorm']['stats-mean'])
        put('bn12.running_var', kw['tdnn12.batchnorm']['stats-var'])
        put('finlin.weight', kw['output.affine']['params'])
        put('finlin.bias', kw['output.affine']['bias'])
        self.invalidate_packed()


def _train_call(ext, lengths, dev):
    """What a training forward starts from -> (U, R, pooling kind, utterance offsets on the device, empty output).
    The copy of the offsets waits for the stream: call this after the host work (packed images), next to the C call."""
    U, R = len(lengths), int(sum(lengths))
    starts = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    out = torch.empty((U, XVEC_DIM), dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        offs = torch.from_numpy(starts).to(dev)
    return U, R, _pool_kind(ext.pooling_function), offs, out


def _split_grad(grad, shapes):
    """The flat gradient of the C ABI -> one view per parameter (`_grad_params` order)."""
    grads, o = [], 0
    for sh in shapes:
        k = int(np.prod(sh))
        grads.append(grad[o:o + k].view(sh))
        o += k
    return tuple(grads)


def _backward(ctx, dout, ws_bytes, backward):
    """One backward call on what the forward kept in ctx.state (dropped here): `ws_bytes` and `backward` name the path's
    C entry points, the state's last entry is its workspace allocator (n, dev) or None.  -> Function.backward's result."""
    saved, offs, packed, packed_t, R, U, kind, dev, shapes, alloc = ctx.state
    lib = _lib.load()
    with _lib.on_device(dev):
        d = dout.detach().to(dev, torch.float32).contiguous()
        grad = torch.empty(lib.nplda_xvec_grad_floats(), dtype=torch.float32, device=dev)
        n = getattr(lib, ws_bytes)(R, U)
        ws = torch.empty(n, dtype=torch.uint8, device=dev) if alloc is None else alloc(n, dev)
        _lib.check(getattr(lib, backward)(saved.data_ptr(), saved.numel(), offs.data_ptr(), U, R, kind, d.data_ptr(),
                                          XVEC_DIM, packed.data_ptr(), packed_t.data_ptr(), grad.data_ptr(),
                                          ws.data_ptr(), n, _lib.current_stream(dev)), backward)
    ctx.state = None
    return (None,) * 5 + _split_grad(grad, shapes)


class _ExtractFn(torch.autograd.Function):
    """extract / extract_ragged with a backward to the 22 tdnn1..tdnn10 / lin11 parameters (inputs after the first
    five, in `_grad_params` order).  The saved buffer (~30 KB per frame) lives from forward to backward."""

    @staticmethod
    def forward(ctx, ext, X, layout, lengths, dev, *params):
        packed, packed_t = ext._packed(dev), ext._packed_t(dev)
        lib = _lib.load()
        U, R, kind, offs, out = _train_call(ext, lengths, dev)
        with _lib.on_device(dev):
            n = lib.nplda_xvec_train_saved_bytes(R, U)
            saved = torch.empty(n, dtype=torch.uint8, device=dev)
            _lib.check(lib.nplda_xvec_extract_train_f32(X.data_ptr(), layout, FEAT, offs.data_ptr(), U, R, kind,
                                                        packed.data_ptr(), out.data_ptr(), XVEC_DIM, saved.data_ptr(), n,
                                                        _lib.current_stream(dev)), "nplda_xvec_extract_train_f32")
        ctx.state = (saved, offs, packed, packed_t, R, U, kind, dev, [tuple(p.shape) for p in params], None)
        return out

    @staticmethod
    def backward(ctx, dout):
        return _backward(ctx, dout, "nplda_xvec_backward_workspace_bytes", "nplda_xvec_backward_f32")


def _bn_buffer(ext, n, dev, what):
    return torch.empty(n, dtype=torch.uint8, device=dev) if ext._bn_alloc is None else ext._bn_alloc(n, dev, what)


def _bn_forward(ext, X, layout, lengths, dev):
    """One nplda_xvec_extract_train_bn_f32 call over the whole batch, then torch's running-statistics update on the
    module's buffers (in-place torch ops, so that the packed-image cache, keyed on their versions, notices).
    -> (x-vectors, (saved, offs, packed, R, U, kind, dev): what _ExtractBnFn keeps for its backward)."""
    packed = ext._packed(dev)
    lib = _lib.load()
    bns = [t.bn for t in ext.tdnns()]
    U, R, kind, offs, out = _train_call(ext, lengths, dev)
    with _lib.on_device(dev):
        n = lib.nplda_xvec_train_bn_saved_bytes(R, U)
        saved = _bn_buffer(ext, n, dev, "saved")
        ns = lib.nplda_xvec_bn_stats_bytes()
        stats = torch.empty(ns, dtype=torch.uint8, device=dev)
        eps = (ctypes.c_float * 10)(*[float(bn.eps) for bn in bns])
        _lib.check(lib.nplda_xvec_extract_train_bn_f32(X.data_ptr(), layout, FEAT, offs.data_ptr(), U, R, kind,
                                                       packed.data_ptr(), eps, out.data_ptr(), XVEC_DIM,
                                                       saved.data_ptr(), n, stats.data_ptr(), ns,
                                                       _lib.current_stream(dev)), "nplda_xvec_extract_train_bn_f32")
        table = stats[:ns - 80].view(torch.float32)  # per layer mean | unbiased variance; ten int64 n_l follow
    with torch.no_grad():
        o = 0
        for bn, (_, dout, _, _) in zip(bns, LAYERS):
            ld = (dout + 15) // 16 * 16
            m = float(bn.momentum)
            mean, var = table[o:o + dout], table[o + ld:o + ld + dout]
            bn.running_mean.mul_(1.0 - m).add_(mean.to(bn.running_mean.device, bn.running_mean.dtype), alpha=m)
            bn.running_var.mul_(1.0 - m).add_(var.to(bn.running_var.device, bn.running_var.dtype), alpha=m)
            if bn.num_batches_tracked is not None:
                bn.num_batches_tracked.add_(1)
            o += 2 * ld
    return out, (saved, offs, packed, R, U, kind, dev)


class _ExtractBnFn(torch.autograd.Function):
    """extract / extract_ragged under batch-statistics batch norm, with a backward to the 22 tdnn1..tdnn10 / lin11
    parameters (`_grad_params` order).  The saved buffer (~31 KB per frame) lives from forward to backward."""

    @staticmethod
    def forward(ctx, ext, X, layout, lengths, dev, *params):
        packed_t = ext._packed_t(dev)  # (before the update of the running statistics drops the cache entry)
        out, kept = _bn_forward(ext, X, layout, lengths, dev)
        ctx.state = kept[:3] + (packed_t,) + kept[3:] + ([tuple(p.shape) for p in params],
                                                         lambda n, dev: _bn_buffer(ext, n, dev, "ws"))
        return out

    @staticmethod
    def backward(ctx, dout):
        return _backward(ctx, dout, "nplda_xvec_backward_bn_workspace_bytes", "nplda_xvec_backward_bn_f32")


class Etdnn_Xvec_NeuralPlda(NeuralPlda):
    """utils/models.py:216-345: the NPLDA head on an E-TDNN extractor.  `nc` is an E2EConf (or any object with its
    xvector_dim, layer1_LDA_dim, layer2_PLDA_spkfactor_dim, pooling_function, beta, alpha, device, loss).  The head's
    parameters, losses, cdet, minc and SaveModel are NeuralPlda's (the same HIP kernels)."""

    def __init__(self, nc):
        super(Etdnn_Xvec_NeuralPlda, self).__init__(nc)
        self.pooling_function = torch.var if getattr(nc, "pooling_function", "std") == 'var' else torch.std
        self.xvector_extractor = XVectorNet_ETDNN_12Layer(pooling_function=self.pooling_function)
        # the reference registers the extractor before the head (state-dict order of its checkpoints)
        mods = self._modules
        self._modules = type(mods)([("xvector_extractor", mods["xvector_extractor"])] +
                                   [(k, v) for k, v in mods.items() if k != "xvector_extractor"])

    def train1(self, finetune_extractor=None):
        """utils/models.py:231-242: training mode with the tdnn batch norms on their running statistics.
        finetune_extractor: None leaves XVectorNet_ETDNN_12Layer.enable_backward's switch as it is; True / False sets it
        (True: a trainable extractor is trained end to end through the HIP backward)."""
        self.train()
        for t in self.xvector_extractor.tdnns():
            t.bn.training = False
        if finetune_extractor is not None:
            self.xvector_extractor.enable_backward(finetune_extractor)
        return self

    def extract_plda_embeddings(self, x):
        """utils/models.py:244-249."""
        return super(Etdnn_Xvec_NeuralPlda, self).extract_plda_embeddings(self.xvector_extractor.extract(x))

    def forward(self, x1, x2):
        """utils/models.py:257-261: features (B, 30, T1), (B, 30, T2) -> scores (B,)."""
        ext = self.xvector_extractor
        return super(Etdnn_Xvec_NeuralPlda, self).forward(ext.extract(x1), ext.extract(x2))

    def LoadParamsFromKaldi(self, xvec_etdnn_pickle_file, mean_vec_file, transform_mat_file, PldaFile):
        """utils/models.py:323-340, the Kaldi files read natively (kaldi_format) as NeuralPlda.LoadPldaParamsFromKaldi."""
        self.xvector_extractor.LoadFromKaldi(xvec_etdnn_pickle_file)
        kaldi_format.fold_init(self, mean_vec_file, transform_mat_file, PldaFile)
