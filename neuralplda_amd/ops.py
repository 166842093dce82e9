"""Thin tensor-level wrappers over the C ABI (include/nplda_hip.h).

Every function takes torch tensors that live on a HIP device, enqueues the kernel on torch's
current stream and returns torch tensors.  No CPU path exists: a CPU tensor is an error here
(neuralplda_amd.models stages CPU inputs through the device, it never computes on the host).
"""
import collections
import ctypes
import functools

import torch

from . import _lib


class PackedParams:
    """MFMA-fragment-ordered image of one parameter set (see csrc/nplda_common.h).  precision: "fp32" (exact
    fp32 MFMA, default) or "bf16x3" (split-bf16 image for the opt-in scoring kernels, csrc/nplda_fwd_bf16x3.h)."""

    __slots__ = ("buf", "D0", "D1", "D2", "ldz", "precision")

    def __init__(self, buf, D0, D1, D2, ldz, precision="fp32"):
        self.buf, self.D0, self.D1, self.D2, self.ldz, self.precision = buf, D0, D1, D2, ldz, precision

    @property
    def device(self):
        return self.buf.device


def _require_dev_f32(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise _lib.NpldaHipError(f"{name} must live on a HIP device (got {t.device}); there is no CPU path")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32 (got {t.dtype})")


def _rows(t, name, D0):
    """Return (tensor, ld) with unit inner stride, 16-byte-aligned rows of at least D0 floats."""
    _require_dev_f32(t, name)
    if t.dim() != 2 or t.shape[1] != D0:
        raise ValueError(f"{name} must have shape (B, {D0}), got {tuple(t.shape)}")
    ok = t.stride(1) == 1 and t.stride(0) >= D0 and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0
    if t.shape[0] <= 1:
        ok = ok or t.is_contiguous() and t.data_ptr() % 16 == 0
    if not ok:
        t = t.contiguous()
        if t.data_ptr() % 16 != 0:  # pragma: no cover (torch allocations are >= 256-B aligned)
            t = t.clone()
    ld = t.stride(0) if t.shape[0] > 1 else max(D0, 4)
    return t, ld


def _pair_rows(x1, x2, D0, n1="x1", n2="x2"):
    """_rows on both sides of a pair batch -> (x1, x2, ld) with ONE row stride: contiguous copies where the two differ."""
    x1, ld1 = _rows(x1, n1, D0)
    x2, ld2 = _rows(x2, n2, D0)
    if ld1 != ld2:
        x1, x2, ld1 = x1.contiguous(), x2.contiguous(), D0
    return x1, x2, ld1


def pack_params(W1, b1, W2, b2, P_sqrt, Q, precision="fp32"):
    """nplda_pack_params_f32 (or nplda_pack_params_bf16x3): nn.Linear-layout parameters -> PackedParams."""
    lib = _lib.load()
    if precision not in ("fp32", "bf16x3"):
        raise ValueError("precision must be 'fp32' or 'bf16x3'")
    for n, t in (("W1", W1), ("b1", b1), ("W2", W2), ("b2", b2), ("P_sqrt", P_sqrt), ("Q", Q)):
        _require_dev_f32(t, n)
    D1, D0 = W1.shape
    D2, D1b = W2.shape
    if D1b != D1 or b1.numel() != D1 or b2.numel() != D2 or P_sqrt.numel() != D2 or Q.numel() != D2:
        raise ValueError("inconsistent parameter shapes")
    if D0 % 4 != 0:
        raise ValueError(f"xvector_dim must be a multiple of 4 (got {D0}); pad the x-vectors")
    b3 = precision == "bf16x3"
    nbytes = (lib.nplda_bf16x3_packed_bytes if b3 else lib.nplda_packed_bytes)(D0, D1, D2)
    if nbytes == 0:
        raise _lib.NpldaHipError(
            f"model {D0}->{D1}->{D2} is outside the compiled kernel set (max dim {lib.nplda_max_dim()})")
    buf = torch.empty(nbytes // 4, dtype=torch.float32, device=W1.device)
    ts = [t.detach().contiguous() for t in (W1, b1, W2, b2, P_sqrt, Q)]
    name = "nplda_pack_params_bf16x3" if b3 else "nplda_pack_params_f32"
    with _lib.on_device(W1.device):
        code = getattr(lib, name)(*[_lib.ptr(t) for t in ts], D0, D1, D2, _lib.ptr(buf), nbytes, _lib.current_stream())
    _lib.check(code, name)
    return PackedParams(buf, D0, D1, D2, lib.nplda_padded_dim(D1, D2), precision)


def score_pairs(x1, x2, packed):
    """nplda_score_pairs_f32: (B, D0), (B, D0) -> (B,) scores.  Two bfloat16 row batches (an extractor's output) go to
    nplda_score_pairs_bf16rows_f32 where the streaming kernels apply — no fp32 copy of the batch — and are widened otherwise;
    the scores are those of the widened rows either way."""
    lib = _lib.load()
    if (x1.dtype == torch.bfloat16 and x2.dtype == torch.bfloat16 and packed.precision == "fp32" and x1.is_cuda and x2.is_cuda
            and x1.dim() == 2 and x1.shape == x2.shape and x1.shape[1] == packed.D0):
        B = x1.shape[0]
        ok = all(t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.data_ptr() % 8 == 0 for t in (x1, x2)) and x1.stride(0) == x2.stride(0)
        if ok and B > 0:
            s = torch.empty(B, dtype=torch.float32, device=x1.device)
            with _lib.on_device(x1.device):
                code = lib.nplda_score_pairs_bf16rows_f32(x1.data_ptr(), x2.data_ptr(), B, x1.stride(0), _lib.ptr(packed.buf),
                                                          packed.D0, packed.D1, packed.D2, _lib.ptr(s), _lib.current_stream())
            if code == 0:
                return s
            if code != _lib.NPLDA_EUNSUPPORTED:
                _lib.check(code, "nplda_score_pairs_bf16rows_f32")
    # any remaining non-fp32 floating input (bf16 rows the streaming form did not take — a 'bf16x3' image, short or
    # strided batches —, fp16, fp64) is widened / narrowed here: the kernels below read fp32 rows
    if torch.is_tensor(x1) and x1.is_floating_point() and x1.dtype != torch.float32:
        x1 = x1.float()
    if torch.is_tensor(x2) and x2.is_floating_point() and x2.dtype != torch.float32:
        x2 = x2.float()
    x1, x2, ld = _pair_rows(x1, x2, packed.D0)
    if x1.shape[0] != x2.shape[0]:
        raise ValueError("x1 and x2 must have the same number of rows")
    B = x1.shape[0]
    s = torch.empty(B, dtype=torch.float32, device=x1.device)
    if B == 0:
        return s
    name = "nplda_score_pairs_bf16x3" if packed.precision == "bf16x3" else "nplda_score_pairs_f32"
    with _lib.on_device(x1.device):
        code = getattr(lib, name)(_lib.ptr(x1), _lib.ptr(x2), B, ld, _lib.ptr(packed.buf), packed.D0, packed.D1, packed.D2,
                                  _lib.ptr(s), _lib.current_stream())
    _lib.check(code, name)
    return s


def score_pairs_rows(table, rows1, rows2, packed):
    """nplda_score_pairs_rows_f32: scores of the pairs (table[rows1], table[rows2]) of a resident (N, D0) x-vector matrix,
    the gather folded into the kernel; falls back to gather_rows + score_pairs where the fused form does not apply."""
    lib = _lib.load()
    if packed.precision != "fp32" or rows1.dtype != torch.int64 or rows2.dtype != torch.int64:
        return score_pairs(gather_rows(table, rows1), gather_rows(table, rows2), packed)
    table, ldt = _rows(table, "table", packed.D0)
    rows1, rows2 = rows1.contiguous(), rows2.contiguous()
    B = rows1.shape[0]
    if rows2.shape[0] != B:
        raise ValueError("rows1 and rows2 must have the same length")
    s = torch.empty(B, dtype=torch.float32, device=table.device)
    if B == 0:
        return s
    with _lib.on_device(table.device):
        code = lib.nplda_score_pairs_rows_f32(_lib.ptr(table), table.shape[0], ldt, _lib.ptr(rows1), _lib.ptr(rows2), B,
                                              _lib.ptr(packed.buf), packed.D0, packed.D1, packed.D2, _lib.ptr(s),
                                              _lib.current_stream())
    if code == _lib.NPLDA_EUNSUPPORTED:  # a shape the balanced-tile kernel does not cover
        return score_pairs(gather_rows(table, rows1), gather_rows(table, rows2), packed)
    _lib.check(code, "nplda_score_pairs_rows_f32")
    return s


def embed(x, packed, want_q=True):
    """nplda_embed_f32: (N, D0) -> z table (N, ldz) [columns >= D2 are zero] and q (N,)."""
    lib = _lib.load()
    x, ld = _rows(x, "x", packed.D0)
    N = x.shape[0]
    z = torch.empty((N, packed.ldz), dtype=torch.float32, device=x.device)
    q = torch.empty(N, dtype=torch.float32, device=x.device) if want_q else None
    if N == 0:
        return z, q
    name = "nplda_embed_bf16x3" if packed.precision == "bf16x3" else "nplda_embed_f32"
    with _lib.on_device(x.device):
        code = getattr(lib, name)(_lib.ptr(x), N, ld, _lib.ptr(packed.buf), packed.D0, packed.D1, packed.D2, _lib.ptr(z),
                                  packed.ldz, _lib.ptr(q), _lib.current_stream())
    _lib.check(code, name)
    return z, q


def embed_rows(table, rows, packed):
    """nplda_embed_rows_f32: embed(table[rows]) -> (z (U, ldz), q (U,)) with the gather folded into the kernel; gather_rows +
    embed where the fused form does not apply (same values)."""
    lib = _lib.load()
    if packed.precision != "fp32" or rows.dtype != torch.int64:
        return embed(gather_rows(table, rows), packed)
    table, ldt = _rows(table, "table", packed.D0)
    rows = rows.contiguous()
    U = rows.shape[0]
    z = torch.empty((U, packed.ldz), dtype=torch.float32, device=table.device)
    q = torch.empty(U, dtype=torch.float32, device=table.device)
    if U == 0:
        return z, q
    with _lib.on_device(table.device):
        code = lib.nplda_embed_rows_f32(_lib.ptr(table), table.shape[0], ldt, _lib.ptr(rows), U, _lib.ptr(packed.buf),
                                        packed.D0, packed.D1, packed.D2, _lib.ptr(z), packed.ldz, _lib.ptr(q),
                                        _lib.current_stream())
    if code == _lib.NPLDA_EUNSUPPORTED:
        return embed(gather_rows(table, rows), packed)
    _lib.check(code, "nplda_embed_rows_f32")
    return z, q


def embed_pair(xa, xb, packed):
    """nplda_embed_pair_f32: the z tables and q vectors of two row sets, ((za, qa), (zb, qb)) — views of ONE (Na + Nb, ldz)
    table filled by one launch where the balanced-tile kernel applies (same values as two embed() calls)."""
    lib = _lib.load()
    if packed.precision != "fp32":
        return embed(xa, packed), embed(xb, packed)
    xa, lda = _rows(xa, "xa", packed.D0)
    xb, ldb = _rows(xb, "xb", packed.D0)
    if lda != ldb or xa.device != xb.device:
        return embed(xa, packed), embed(xb, packed)
    Na, Nb = xa.shape[0], xb.shape[0]
    z = torch.empty((Na + Nb, packed.ldz), dtype=torch.float32, device=xa.device)
    q = torch.empty(Na + Nb, dtype=torch.float32, device=xa.device)
    if Na + Nb > 0:
        with _lib.on_device(xa.device):
            code = lib.nplda_embed_pair_f32(_lib.ptr(xa), Na, _lib.ptr(xb), Nb, lda, _lib.ptr(packed.buf), packed.D0, packed.D1,
                                            packed.D2, _lib.ptr(z), packed.ldz, _lib.ptr(q), _lib.current_stream())
        _lib.check(code, "nplda_embed_pair_f32")
    return (z[:Na], q[:Na]), (z[Na:], q[Na:])


# ---- training ---------------------------------------------------------------------------------

LOSS_SOFTCDET, LOSS_BCE, LOSS_HARD_CDET = 0, 1, 2


def _need_fp32(packed, what):
    if packed.precision != "fp32":
        raise ValueError(f"{what} needs the fp32 parameter image (pack_params(..., precision='fp32'))")


def forward_train(x1, x2, packed):
    """nplda_forward_train_f32: scores plus the activations the backward needs.
    Returns (s, saved) with saved = (x1, x2, ld, y, z, rn) device tensors."""
    lib = _lib.load()
    _need_fp32(packed, "forward_train")
    x1, x2, ld = _pair_rows(x1, x2, packed.D0)
    if x1.shape[0] != x2.shape[0]:
        raise ValueError("x1 and x2 must have the same number of rows")
    B = x1.shape[0]
    dev = x1.device
    s = torch.empty(B, dtype=torch.float32, device=dev)
    y = torch.empty((2 * B, packed.ldz), dtype=torch.float32, device=dev)
    z = torch.empty((2 * B, packed.ldz), dtype=torch.float32, device=dev)
    rn = torch.empty(2 * B, dtype=torch.float32, device=dev)
    if B > 0:
        with _lib.on_device(dev):
            code = lib.nplda_forward_train_f32(_lib.ptr(x1), _lib.ptr(x2), B, ld, _lib.ptr(packed.buf), packed.D0,
                                               packed.D1, packed.D2, _lib.ptr(s), _lib.ptr(y), _lib.ptr(z),
                                               _lib.ptr(rn), packed.ldz, _lib.current_stream())
        _lib.check(code, "nplda_forward_train_f32")
    return s, (x1, x2, ld, y, z, rn)


@functools.lru_cache(maxsize=64)
def _backward_sizes(rows, D0, D1, D2, want_dx):
    lib = _lib.load()
    return (lib.nplda_grad_floats(D0, D1, D2), lib.nplda_backward_ex_workspace_bytes(rows, D0, D1, D2, want_dx))


def backward(saved, g, packed, P_sqrt, want_dx=False):
    """nplda_backward_ex_f32: flat gradient [dW1 | db1 | dW2 | db2 | dP_sqrt | dQ] for dL/ds = g; with want_dx also
    the input gradients -> (flat, dx1, dx2), dx (B, D0) = du . W1."""
    lib = _lib.load()
    x1, x2, ld, y, z, rn = saved
    B = x1.shape[0]
    dev = x1.device
    _require_dev_f32(g, "g")
    g = g.contiguous()
    n, wsb = _backward_sizes(2 * B, packed.D0, packed.D1, packed.D2, 1 if want_dx else 0)
    flat = torch.empty(n, dtype=torch.float32, device=dev)
    ws = torch.empty(max(wsb // 4, 4), dtype=torch.float32, device=dev)
    ps = P_sqrt.detach().contiguous()
    dx1 = torch.empty((B, packed.D0), dtype=torch.float32, device=dev) if want_dx else None
    dx2 = torch.empty((B, packed.D0), dtype=torch.float32, device=dev) if want_dx else None
    with _lib.on_device(dev):
        code = lib.nplda_backward_ex_f32(_lib.ptr(x1), _lib.ptr(x2), B, ld, _lib.ptr(packed.buf), packed.D0, packed.D1,
                                         packed.D2, _lib.ptr(g), _lib.ptr(y), _lib.ptr(z), _lib.ptr(rn), packed.ldz,
                                         _lib.ptr(ps), _lib.ptr(ws), wsb, _lib.ptr(flat), _lib.ptr(dx1), _lib.ptr(dx2),
                                         packed.D0, _lib.current_stream())
    _lib.check(code, "nplda_backward_ex_f32")
    return (flat, dx1, dx2) if want_dx else flat


def embed_train(x, packed):
    """nplda_embed_train_f32: (N, D0) -> z (N, ldz) plus the saved rows (x, ld, y (N, ldz), rn (N)) of its backward."""
    lib = _lib.load()
    _need_fp32(packed, "embed_train")
    x, ld = _rows(x, "x", packed.D0)
    N = x.shape[0]
    dev = x.device
    z = torch.empty((N, packed.ldz), dtype=torch.float32, device=dev)
    y = torch.empty((N, packed.ldz), dtype=torch.float32, device=dev)
    rn = torch.empty(N, dtype=torch.float32, device=dev)
    if N > 0:
        with _lib.on_device(dev):
            code = lib.nplda_embed_train_f32(_lib.ptr(x), N, ld, _lib.ptr(packed.buf), packed.D0, packed.D1, packed.D2,
                                             _lib.ptr(z), _lib.ptr(y), _lib.ptr(rn), packed.ldz, _lib.current_stream())
        _lib.check(code, "nplda_embed_train_f32")
    return z, (x, ld, y, rn)


def embed_backward(saved, gz, packed, want_dx=False):
    """nplda_embed_backward_f32: gz = dL/dz (N, D2) -> (flat gradient with dP_sqrt = dQ = 0, dx (N, D0) or None)."""
    lib = _lib.load()
    x, ld, y, rn = saved
    N = x.shape[0]
    dev = x.device
    _require_dev_f32(gz, "gz")
    if gz.dim() != 2 or gz.shape != (N, packed.D2):
        raise ValueError(f"gz must be ({N}, {packed.D2})")
    if gz.stride(1) != 1 or (N > 1 and gz.stride(0) < packed.D2):
        gz = gz.contiguous()
    n = lib.nplda_grad_floats(packed.D0, packed.D1, packed.D2)
    flat = torch.empty(n, dtype=torch.float32, device=dev)
    wsb = lib.nplda_backward_ex_workspace_bytes(N, packed.D0, packed.D1, packed.D2, 1 if want_dx else 0)
    ws = torch.empty(max(wsb // 4, 4), dtype=torch.float32, device=dev)
    dx = torch.empty((N, packed.D0), dtype=torch.float32, device=dev) if want_dx else None
    with _lib.on_device(dev):
        code = lib.nplda_embed_backward_f32(_lib.ptr(x), N, ld, _lib.ptr(packed.buf), packed.D0, packed.D1, packed.D2,
                                            _lib.ptr(gz), gz.stride(0) if N > 1 else packed.D2, _lib.ptr(y),
                                            _lib.ptr(rn), packed.ldz, _lib.ptr(ws), wsb, _lib.ptr(flat), _lib.ptr(dx),
                                            packed.D0, _lib.current_stream())
    _lib.check(code, "nplda_embed_backward_f32")
    return flat, dx


def score_embeddings_bwd(z1, z2, P_sqrt, Q, g, want_dz1=True, want_dz2=True):
    """nplda_score_embeddings_bwd_f32 -> (dz1 or None, dz2 or None, dP_sqrt (D2), dQ (D2))."""
    lib = _lib.load()
    for n, t in (("z1", z1), ("z2", z2), ("P_sqrt", P_sqrt), ("Q", Q), ("g", g)):
        _require_dev_f32(t, n)
    D2 = Q.numel()
    if z1.stride(1) != 1:
        z1 = z1.contiguous()
    if z2.stride(1) != 1:
        z2 = z2.contiguous()
    B = z1.shape[0]
    dev = z1.device
    dz1 = torch.empty((B, D2), dtype=torch.float32, device=dev) if want_dz1 else None
    dz2 = torch.empty((B, D2), dtype=torch.float32, device=dev) if want_dz2 else None
    dP = torch.empty(D2, dtype=torch.float32, device=dev)
    dQ = torch.empty(D2, dtype=torch.float32, device=dev)
    wsb = lib.nplda_score_embeddings_bwd_workspace_bytes(B, D2)
    if wsb == 0:
        raise _lib.NpldaHipError(f"embedding dimension {D2} is outside the compiled kernel set")
    ws = torch.empty(wsb // 4, dtype=torch.float32, device=dev)
    ld1 = z1.stride(0) if B > 1 else D2
    ld2 = z2.stride(0) if B > 1 else D2
    with _lib.on_device(dev):
        code = lib.nplda_score_embeddings_bwd_f32(_lib.ptr(z1), ld1, _lib.ptr(z2), ld2, B, D2,
                                                  _lib.ptr(P_sqrt.contiguous()), _lib.ptr(Q.contiguous()),
                                                  _lib.ptr(g.contiguous()), _lib.ptr(dz1), D2, _lib.ptr(dz2), D2,
                                                  _lib.ptr(dP), _lib.ptr(dQ), _lib.ptr(ws), wsb, _lib.current_stream())
    _lib.check(code, "nplda_score_embeddings_bwd_f32")
    return dz1, dz2, dP, dQ


def pack_matrix(src, mode=0):
    """nplda_pack_matrix_f32: fragment image of Wm = src (mode 0), src^T (1) or src + src^T (2) -> (frag, K, N)."""
    lib = _lib.load()
    _require_dev_f32(src, "src")
    if src.dim() != 2 or src.stride(1) != 1:
        raise ValueError("src must be a 2-D tensor with unit inner stride")
    K, N = (src.shape[1], src.shape[0]) if mode == 1 else (src.shape[0], src.shape[1])
    nbytes = lib.nplda_matrix_frag_bytes(K, N)
    if nbytes == 0:
        raise _lib.NpldaHipError(f"a {K} x {N} matrix is outside the resident-matrix GEMM (K <= 512, N % 4 == 0)")
    frag = torch.empty(nbytes // 4, dtype=torch.float32, device=src.device)
    with _lib.on_device(src.device):
        code = lib.nplda_pack_matrix_f32(_lib.ptr(src), src.stride(0), K, N, mode, _lib.ptr(frag), nbytes,
                                         _lib.current_stream())
    _lib.check(code, "nplda_pack_matrix_f32")
    return frag, K, N


def rows_matmul(rows, packed_matrix, bias=None, rowscale=None):
    """nplda_rows_matmul_f32: out[r] = rowscale[r] * (rows[r, :K] . Wm + bias) -> (R, N)."""
    lib = _lib.load()
    frag, K, N = packed_matrix
    rows, ld = _rows(rows, "rows", K)
    R = rows.shape[0]
    out = torch.empty((R, N), dtype=torch.float32, device=rows.device)
    if R == 0:
        return out
    with _lib.on_device(rows.device):
        code = lib.nplda_rows_matmul_f32(_lib.ptr(rows), ld, R, K, _lib.ptr(frag), N,
                                         _lib.ptr(bias.contiguous()) if bias is not None else None,
                                         _lib.ptr(rowscale.contiguous()) if rowscale is not None else None,
                                         _lib.ptr(out), N, _lib.current_stream())
    _lib.check(code, "nplda_rows_matmul_f32")
    return out


def lda_backward(x1, x2, paired, rn, dpaired, W1, want_w=True, want_dx=True):
    """Backward through y = normalize(LDA x) of a paired-row head (DPlda): dpaired = dL/d[y1 | y2] (B, 2 D1) ->
    (dW1 (D1, D0), db1 (D1), dx1, dx2): F.normalize backward on the paired rows, then the wgrad / dgrad GEMMs."""
    lib = _lib.load()
    D1, D0 = W1.shape
    x1, x2, ld = _pair_rows(x1, x2, D0)
    B = x1.shape[0]
    dev = x1.device
    Mp = lib.nplda_padded_dim(D1, D1)
    du = torch.empty((2 * B, Mp), dtype=torch.float32, device=dev)
    dW1 = db1 = dx1 = dx2 = None
    st = _lib.current_stream()
    with _lib.on_device(dev):
        _lib.check(lib.nplda_normalize_bwd_paired_f32(_lib.ptr(dpaired), dpaired.stride(0), _lib.ptr(paired),
                                                      paired.stride(0), _lib.ptr(rn), B, D1, _lib.ptr(du), Mp, st),
                   "nplda_normalize_bwd_paired_f32")
        if want_w:
            wsb = lib.nplda_lda_wgrad_workspace_bytes(B, D0, D1)
            ws = torch.empty(max(wsb // 4, 4), dtype=torch.float32, device=dev)
            out = torch.empty(D1 * D0 + D1, dtype=torch.float32, device=dev)
            _lib.check(lib.nplda_lda_wgrad_f32(_lib.ptr(x1), _lib.ptr(x2), B, ld, _lib.ptr(du), Mp, D0, D1,
                                               _lib.ptr(ws), wsb, _lib.ptr(out), st), "nplda_lda_wgrad_f32")
            dW1, db1 = out[:D1 * D0].view(D1, D0), out[D1 * D0:]
        if want_dx:
            wsb = lib.nplda_lda_dgrad_workspace_bytes(D0, D1)
            ws = torch.empty(max(wsb // 4, 4), dtype=torch.float32, device=dev)
            dx1 = torch.empty((B, D0), dtype=torch.float32, device=dev)
            dx2 = torch.empty((B, D0), dtype=torch.float32, device=dev)
            _lib.check(lib.nplda_lda_dgrad_f32(_lib.ptr(du), Mp, B, _lib.ptr(W1.detach().contiguous()), D0, D1,
                                               _lib.ptr(ws), wsb, _lib.ptr(dx1), _lib.ptr(dx2), D0, st),
                       "nplda_lda_dgrad_f32")
    return dW1, db1, dx1, dx2


def split_flat_grad(flat, D0, D1, D2):
    """Views (dW1, db1, dW2, db2, dP_sqrt, dQ) into the flat gradient buffer."""
    w1, b1, w2, b2, ps, q = flat.split_with_sizes((D1 * D0, D1, D2 * D1, D2, D2, D2))  # (one call: six views)
    return w1.view(D1, D0), b1, w2.view(D2, D1), b2, ps, q


def _theta_array(thetas):
    arr = (ctypes.c_void_p * len(thetas))()
    for i, t in enumerate(thetas):
        _require_dev_f32(t, "theta")
        arr[i] = t.data_ptr()
    return arr


def _step_consts(params, thetas, betas, kind):
    """The ctypes arrays of one call -> (parr, tharr, barr, K): the six parameter pointers (None for `params` None: the
    loss entry points take none), the K threshold pointers and the K betas (None for BCE, which has none).  Built on
    every call: a captured graph keeps the pointers, not these arrays."""
    K = len(thetas)
    parr = (ctypes.c_void_p * 6)(*[q.data_ptr() for q in params]) if params is not None else None
    barr = (ctypes.c_float * max(K, 1))(*[float(b) for b in betas]) if kind != LOSS_BCE else None
    return parr, _theta_array(thetas), barr, K


def loss_sums(s, t, thetas, alpha, kind):
    """nplda_loss_sums_f32: fp64 vector of batch-global sums (additive across shards)."""
    lib = _lib.load()
    _require_dev_f32(s, "output")
    _require_dev_f32(t, "target")
    s, t = s.contiguous(), t.contiguous()
    if s.shape != t.shape or s.dim() != 1:
        raise ValueError("output and target must be 1-D tensors of the same length")
    K = len(thetas)
    ns = lib.nplda_loss_nsums(K, kind)
    if ns == 0:
        raise _lib.NpldaHipError(f"loss with {K} thresholds is not supported by the compiled kernels (max 4)")
    sums = torch.empty(ns, dtype=torch.float64, device=s.device)
    with _lib.on_device(s.device):
        code = lib.nplda_loss_sums_f32(_lib.ptr(s), _lib.ptr(t), s.shape[0], _theta_array(thetas), K, float(alpha),
                                       kind, _lib.ptr(sums), _lib.current_stream())
    _lib.check(code, "nplda_loss_sums_f32")
    return sums


def loss_finish(s, t, thetas, betas, alpha, kind, sums, want_grad=True):
    """nplda_loss_finish_f32: (loss 0-d tensor, g or None, dtheta (K,) or None)."""
    lib = _lib.load()
    s, t = s.contiguous(), t.contiguous()
    K = len(thetas)
    dev = s.device
    loss = torch.empty((), dtype=torch.float32, device=dev)
    g = torch.empty_like(s) if want_grad else None
    dth = torch.empty(K, dtype=torch.float32, device=dev) if want_grad else None
    _, tharr, barr, _ = _step_consts(None, thetas, betas, kind)
    with _lib.on_device(dev):
        code = lib.nplda_loss_finish_f32(_lib.ptr(s), _lib.ptr(t), s.shape[0], tharr, barr, K,
                                         float(alpha), kind, _lib.ptr(sums), _lib.ptr(loss), _lib.ptr(g),
                                         _lib.ptr(dth), _lib.current_stream())
    _lib.check(code, "nplda_loss_finish_f32")
    return loss, g, dth


def loss_fwd_bwd(s, t, thetas, betas, alpha, kind, want_joint=False):
    """nplda_loss_fwd_bwd_f32: (loss 0-d tensor, g, dtheta (K,), sums[, the buffer g and dtheta live in]) of an unsharded batch — both loss passes in one
    call (one launch up to 4096 pairs), bit-identical to loss_sums + loss_finish."""
    lib = _lib.load()
    _require_dev_f32(s, "output")
    _require_dev_f32(t, "target")
    s, t = s.contiguous(), t.contiguous()
    if s.shape != t.shape or s.dim() != 1:
        raise ValueError("output and target must be 1-D tensors of the same length")
    K = len(thetas)
    ns = lib.nplda_loss_nsums(K, kind)
    if ns == 0 or kind == LOSS_HARD_CDET:
        raise _lib.NpldaHipError("loss_fwd_bwd: unsupported loss kind / number of thresholds")
    dev = s.device
    sums = torch.empty(ns, dtype=torch.float64, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    # g and dtheta share a buffer ([g (B) | pad to 4 | dtheta (K)]: loss_joint_views): the backward scales both by the
    # incoming dL/dloss with ONE product
    B = s.shape[0]
    joint = torch.empty(((B + 3) & ~3) + K, dtype=torch.float32, device=dev)
    g, dth = loss_joint_views(joint, B, K)
    _, tharr, barr, _ = _step_consts(None, thetas, betas, kind)
    with _lib.on_device(dev):
        code = lib.nplda_loss_fwd_bwd_f32(_lib.ptr(s), _lib.ptr(t), s.shape[0], tharr, barr, K,
                                          float(alpha), kind, _lib.ptr(sums), _lib.ptr(loss), _lib.ptr(g),
                                          _lib.ptr(dth), _lib.current_stream())
    _lib.check(code, "nplda_loss_fwd_bwd_f32")
    return (loss, g, dth, sums, joint) if want_joint else (loss, g, dth, sums)


def loss_joint_views(joint, B, K):
    """(g, dtheta) inside loss_fwd_bwd's joint buffer (or a product of it)."""
    o = (B + 3) & ~3
    return joint[:B], joint[o:o + K]


ALLPAIRS_TILE = 64  # rows of z one block of the all-pairs kernel owns (NPLDA_ALLPAIRS_TILE, include/nplda_hip.h)


def _labels(t, name, N, dev):
    """Integer labels (a tensor on any device, or a sequence of ints) -> contiguous int32 (N,) on `dev`."""
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(t)
        if t.numel() == 0:  # (an empty sequence has no dtype of its own)
            t = t.to(torch.int32)
    if t.is_floating_point() or t.dtype == torch.bool or t.is_complex():
        raise TypeError(f"{name} must be integer labels (got {t.dtype})")
    if t.dim() != 1 or t.shape[0] != N:
        raise ValueError(f"{name} must be one label per row of z: ({N},), got {tuple(t.shape)}")
    if t.dtype != torch.int32:
        t = t.to(torch.int32)
    if t.device != dev:
        t = t.to(dev, non_blocking=True)
    return t.contiguous()


def allpairs_loss(z, spk, P_sqrt, Q, thetas, betas, alpha, kind, grp=None, want_grad=True):
    """nplda_allpairs_loss_f32: the loss over every trial (i < j, same group) of the batch z (N, D2) with speaker labels
    spk (N,) -> (loss 0-d, dtheta (K,) or None, sums fp64, dz (N, D2) or None, dP_sqrt (D2) or None, dQ (D2) or None).
    The N x N scores are never materialised; want_grad=False computes the loss and the sums only."""
    lib = _lib.load()
    for n, t in (("z", z), ("P_sqrt", P_sqrt), ("Q", Q)):
        _require_dev_f32(t, n)
    D2 = Q.numel()
    if z.dim() != 2 or z.shape[1] != D2 or P_sqrt.numel() != D2:
        raise ValueError(f"z must be (N, {D2}) and P_sqrt ({D2},)")
    if kind not in (LOSS_SOFTCDET, LOSS_BCE):
        raise _lib.NpldaHipError("allpairs_loss: the loss is SoftCdet or BCE")
    N, dev = z.shape[0], z.device
    K = len(thetas)
    ld = (D2 + 3) & ~3
    if not (z.stride(1) == 1 and z.stride(0) >= D2 and z.stride(0) % 4 == 0 and z.data_ptr() % 16 == 0) and N > 0:
        zb = torch.empty((N, ld), dtype=torch.float32, device=dev)  # 16-byte aligned rows; columns >= D2 are never read
        zb[:, :D2] = z
        z = zb
    spk = _labels(spk, "spk", N, dev)
    grp = None if grp is None else _labels(grp, "grp", N, dev)
    wsb = lib.nplda_allpairs_workspace_bytes(N, D2, K)
    ns = lib.nplda_loss_nsums(K, kind)
    if wsb == 0 or ns == 0:
        raise _lib.NpldaHipError(f"allpairs_loss: N = {N}, D2 = {D2}, K = {K} is outside the compiled kernel set")
    ws = torch.empty(wsb // 4, dtype=torch.float32, device=dev)
    sums = torch.empty(ns, dtype=torch.float64, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    dth = dzb = dP = dQ = None
    if want_grad:
        dth = torch.empty(K, dtype=torch.float32, device=dev)
        dzb = torch.empty((N, ld), dtype=torch.float32, device=dev)
        dP = torch.empty(D2, dtype=torch.float32, device=dev)
        dQ = torch.empty(D2, dtype=torch.float32, device=dev)
    _, tharr, barr, _ = _step_consts(None, thetas, betas, kind)
    with _lib.on_device(dev):
        code = lib.nplda_allpairs_loss_f32(_lib.ptr(z), z.stride(0) if N > 1 else ld, N, D2, _lib.ptr(spk), _lib.ptr(grp),
                                           _lib.ptr(P_sqrt.contiguous()), _lib.ptr(Q.contiguous()), tharr, barr, K,
                                           float(alpha), kind, _lib.ptr(sums), _lib.ptr(loss), _lib.ptr(dth),
                                           _lib.ptr(dzb), ld, _lib.ptr(dP), _lib.ptr(dQ), _lib.ptr(ws), wsb,
                                           _lib.current_stream())
    _lib.check(code, "nplda_allpairs_loss_f32")
    if N == 0:  # the call is a no-op there: the formulas on an empty trial set
        sums.zero_()
        loss.fill_(float("nan"))
        for t in (dth, dzb, dP, dQ):
            if t is not None:
                t.zero_()
    return loss, dth, sums, (dzb[:, :D2] if want_grad else None), dP, dQ


CLASSIFY_KINDS = {"softmax": 0, "am": 1, "aam": 2}  # the `kind` of nplda_classify_loss_f32

ClassifyResult = collections.namedtuple("ClassifyResult", "loss counts rowloss pred dx dw db")


def _rows16(t, D):
    """`t` (n, D) as the kernels take a matrix: unit column stride, 16-byte aligned rows of a stride that is a multiple of 4."""
    if t.shape[0] == 0 or (t.stride(1) == 1 and t.stride(0) >= D and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0):
        return t
    buf = torch.empty((t.shape[0], (D + 3) & ~3), dtype=torch.float32, device=t.device)  # columns >= D are never read
    buf[:, :D] = t
    return buf[:, :D]


def classify_loss(x, labels, W, bias=None, kind="aam", scale=30.0, margin=0.2, want_dx=True, want_dw=True, class_chunks=0,
                  row_chunks=0):
    """nplda_classify_loss_f32: softmax ("softmax"), AM-softmax ("am") or AAM-softmax ("aam") cross entropy of the embeddings
    x (N, D) against the class table W (C, D) with optional bias (C,) and integer labels (N,) (-1 = ignore the row)
    -> ClassifyResult(loss 0-d, counts (3,) int64 = (rows counted, of them classified right, labels out of range),
    rowloss (N,), pred (N,) int32 = argmax of the margin-free logits, dx (N, D) or None, dw (C, D) or None, db (C,) or None
    (with want_dw, when there is a bias)).  The N x C logits are never materialised.  class_chunks / row_chunks: 0 = the
    plan's choice."""
    lib = _lib.load()
    _require_dev_f32(x, "x")
    _require_dev_f32(W, "W")
    if kind not in CLASSIFY_KINDS:
        raise ValueError(f"classify_loss: kind is one of {sorted(CLASSIFY_KINDS)}, got {kind!r}")
    if x.dim() != 2 or W.dim() != 2 or x.shape[1] != W.shape[1]:
        raise ValueError(f"x must be (N, D) and W (C, D), got {tuple(x.shape)} and {tuple(W.shape)}")
    (N, D), C, dev = x.shape, W.shape[0], x.device
    if bias is not None:
        _require_dev_f32(bias, "bias")
        if bias.shape != (C,):
            raise ValueError(f"bias must be ({C},), got {tuple(bias.shape)}")
        bias = bias.contiguous()
    y = _labels(labels, "labels", N, dev)
    x, W = _rows16(x, D), _rows16(W, D)
    ld = (D + 3) & ~3
    wsb = lib.nplda_classify_workspace_bytes(N, C, D, class_chunks, row_chunks)
    if wsb == 0:
        raise _lib.NpldaHipError(f"classify_loss: N = {N}, C = {C}, D = {D} is outside the compiled kernel set")
    ws = torch.empty(wsb // 4, dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    counts = torch.empty(3, dtype=torch.int64, device=dev)
    rowloss = torch.empty(N, dtype=torch.float32, device=dev)
    pred = torch.empty(N, dtype=torch.int32, device=dev)
    dxb = torch.empty((N, ld), dtype=torch.float32, device=dev) if want_dx else None
    dwb = torch.empty((C, ld), dtype=torch.float32, device=dev) if want_dw else None
    db = torch.empty(C, dtype=torch.float32, device=dev) if want_dw and bias is not None else None
    with _lib.on_device(dev):
        code = lib.nplda_classify_loss_f32(_lib.ptr(x), x.stride(0) if N > 1 else ld, N, _lib.ptr(W),
                                           W.stride(0) if C > 1 else ld, C, D, _lib.ptr(bias), _lib.ptr(y),
                                           CLASSIFY_KINDS[kind], float(scale), float(margin), class_chunks, row_chunks,
                                           _lib.ptr(loss), _lib.ptr(counts), _lib.ptr(rowloss), _lib.ptr(pred),
                                           _lib.ptr(dxb), ld, _lib.ptr(dwb), ld, _lib.ptr(db), _lib.ptr(ws), wsb,
                                           _lib.current_stream())
    _lib.check(code, "nplda_classify_loss_f32")
    if N == 0 or C == 0:  # the call is a no-op there: the formulas on an empty problem
        loss.fill_(float("nan"))
        counts.zero_()
        rowloss.zero_()
        pred.zero_()
        for t in (dxb, dwb, db):
            if t is not None:
                t.zero_()
    return ClassifyResult(loss, counts, rowloss, pred, None if dxb is None else dxb[:, :D],
                          None if dwb is None else dwb[:, :D], db)


def pack_params_into(packed, W1, b1, W2, b2, P_sqrt, Q):
    """nplda_pack_params_f32 into an EXISTING PackedParams buffer (its address is baked into captured graphs)."""
    lib = _lib.load()
    _need_fp32(packed, "pack_params_into")
    ts = [t.detach().contiguous() for t in (W1, b1, W2, b2, P_sqrt, Q)]
    for n, t in zip(("W1", "b1", "W2", "b2", "P_sqrt", "Q"), ts):
        _require_dev_f32(t, n)
    with _lib.on_device(packed.buf.device):
        code = lib.nplda_pack_params_f32(*[_lib.ptr(t) for t in ts], packed.D0, packed.D1, packed.D2, _lib.ptr(packed.buf),
                                         packed.buf.numel() * 4, _lib.current_stream())
    _lib.check(code, "nplda_pack_params_f32")
    return packed


def repack_params(packed, keys):
    """The image of `packed` refreshed from six parameter tensors that were validated when it was first packed (same
    storage, same device: `keys` = their (data_ptr, version, device) triples) — the raw launch, nothing else."""
    lib = _lib.load()
    name = "nplda_pack_params_bf16x3" if packed.precision == "bf16x3" else "nplda_pack_params_f32"
    dev = keys[0][2]
    with _lib.on_device(dev):
        code = getattr(lib, name)(keys[0][0], keys[1][0], keys[2][0], keys[3][0], keys[4][0], keys[5][0], packed.D0, packed.D1,
                                  packed.D2, packed.buf.data_ptr(), packed.buf.numel() * 4, _lib.current_stream())
    _lib.check(code, name)
    return packed


def train_step_workspace(B, packed, rows=False):
    """Workspace tensor for train_step (rows=True: train_step_rows) at batch size B (None when the fused step does not
    cover this size / shape)."""
    lib = _lib.load()
    fn = lib.nplda_train_step_rows_workspace_bytes if rows else lib.nplda_train_step_workspace_bytes
    n = fn(B, packed.D0, packed.D1, packed.D2)
    if n == 0:
        return None
    return torch.empty(n // 4, dtype=torch.float32, device=packed.buf.device)


# The fused train-step family funnels into one C function (train_step_impl, csrc/nplda_backward.hip); its wrappers share
# the helpers below.  Every helper is a pure function of its arguments — train.py bakes the pointers of one call into a
# captured graph, so nothing here may be cached between calls.  What a variant does NOT check is part of what it accepts:
# the gradient forms leave the parameter tensors unchecked, train_step_apply checks nothing but the image's precision, the
# dx forms reject the rows and targets the other forms copy.

def _aligned_target(target, strict=None):
    """The target vector as the kernels read it — device fp32, contiguous, 16-byte aligned: a copy where it is not, or
    with `strict` (the name of a dx form, for the message) an error."""
    _require_dev_f32(target, "target")
    if strict is not None:
        if not target.is_contiguous() or target.data_ptr() % 16:
            raise ValueError(f"{strict}: target must be contiguous and 16-byte aligned")
        return target
    target = target.contiguous()
    return target.clone() if target.data_ptr() % 16 else target


def _dx_rows(what, packed, x1, x2, dx1, dx2, target):
    """The dx forms take x1 / x2 / dx1 / dx2 as they are (float32 or bfloat16, nothing copied) -> (B, io_bf16)."""
    for t in (x1, x2, dx1, dx2):
        if t.dtype != x1.dtype or t.dtype not in (torch.float32, torch.bfloat16) or not t.is_cuda:
            raise ValueError(f"{what}: x1, x2, dx1, dx2 must be device tensors, all float32 or all bfloat16")
        if t.dim() != 2 or t.shape[1] != packed.D0 or t.stride(1) != 1 or t.stride(0) % 4 or t.data_ptr() % 16:
            raise ValueError(f"{what}: (B, D0) rows with unit inner stride, 16-byte aligned")
    B = x1.shape[0]
    if x2.shape[0] != B or target.shape[0] != B or dx1.shape[0] != B or dx2.shape[0] != B:
        raise ValueError("x1, x2, target, dx1, dx2 must have the same number of rows")
    if x1.stride(0) != x2.stride(0) or dx1.stride(0) != dx2.stride(0):
        raise ValueError(f"{what}: x1 / x2 (and dx1 / dx2) must share their row stride")
    return B, 1 if x1.dtype == torch.bfloat16 else 0


def _index_rows(rows1, rows2, target, dev):
    """The rows forms' index vectors: int64 on the table's device, as long as the target -> (rows1, rows2, B)."""
    if rows1.dtype != torch.int64 or rows2.dtype != torch.int64 or rows1.device != dev or rows2.device != dev:
        raise TypeError("rows must be int64 tensors on the table's device")
    rows1, rows2 = rows1.contiguous(), rows2.contiguous()
    B = rows1.shape[0]
    if rows2.shape[0] != B or target.shape[0] != B:
        raise ValueError("rows1, rows2 and target must have the same length")
    return rows1, rows2, B


def _check_global_counts(global_counts):
    if global_counts is not None and (global_counts.dtype != torch.float64 or not global_counts.is_cuda
                                      or global_counts.numel() != 2 or not global_counts.is_contiguous()):
        raise ValueError("global_counts must be a contiguous device float64 tensor [N_t, N_n]")


def _check_flat(flat, packed):
    if flat.dtype != torch.float32 or not flat.is_cuda or flat.numel() < train_step_flat_floats(packed) or not flat.is_contiguous():
        raise ValueError("flat must be a contiguous device float32 tensor of train_step_flat_floats(packed) elements")


def _check_inplace_params(params, thetas, what):
    for q in list(params) + list(thetas):
        _require_dev_f32(q, "parameter")
        if not q.is_contiguous():
            raise ValueError(f"{what} updates the parameter tensors in place: they must be contiguous")


def _floats(*values):
    return [float(v) for v in values]


def train_step(x1, x2, target, params, thetas, betas, alpha, kind, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps,
               weight_decay, packed, ws, loss, grad_out=None, loss_sum=None):
    """nplda_train_step_f32: forward -> loss -> backward -> Adam on `params` (the six parameter tensors, updated IN
    PLACE) and `thetas`, `packed` refreshed to the updated parameters, `loss` (0-d device tensor) written; `loss_sum` (optional 1-element fp64 device tensor) += loss.  Three launches."""
    lib = _lib.load()
    _need_fp32(packed, "train_step")
    x1, x2, ld = _pair_rows(x1, x2, packed.D0)
    if x1.shape[0] != x2.shape[0] or target.shape[0] != x1.shape[0]:
        raise ValueError("x1, x2 and target must have the same number of rows")
    target = _aligned_target(target)
    _check_inplace_params(params, thetas, "train_step")
    parr, tharr, barr, K = _step_consts(params, thetas, betas, kind)
    with _lib.on_device(x1.device):
        code = lib.nplda_train_step_f32(_lib.ptr(x1), _lib.ptr(x2), x1.shape[0], ld, _lib.ptr(target), parr, packed.D0,
                                        packed.D1, packed.D2, tharr, barr, K, float(alpha), kind, _lib.ptr(exp_avg),
                                        _lib.ptr(exp_avg_sq), _lib.ptr(step), *_floats(lr, beta1, beta2, eps, weight_decay),
                                        _lib.ptr(packed.buf), _lib.ptr(ws), ws.numel() * 4, _lib.ptr(loss),
                                        _lib.ptr(loss_sum), _lib.ptr(grad_out), _lib.current_stream())
    _lib.check(code, "nplda_train_step_f32")
    return loss


def train_step_flat_floats(packed):
    """Length of the data-parallel step's flat buffer: the flat gradient + 4 x 18 floats of loss sums (16-bit limbs)."""
    return int(_lib.load().nplda_train_step_flat_floats(packed.D0, packed.D1, packed.D2))


def train_step_grad(x1, x2, target, params, thetas, betas, alpha, kind, step, packed, ws, flat, global_counts=None):
    """nplda_train_step_grad_f32: this rank's share of a data-parallel step up to the flat gradient (+ loss sums) in
    `flat`; `global_counts` = device float64 [N_t, N_n] of the GLOBAL minibatch (None: one rank).  Follow with a SUM
    all-reduce of `flat` and train_step_apply."""
    lib = _lib.load()
    _need_fp32(packed, "train_step_grad")
    x1, x2, ld = _pair_rows(x1, x2, packed.D0)
    if x1.shape[0] != x2.shape[0] or target.shape[0] != x1.shape[0]:
        raise ValueError("x1, x2 and target must have the same number of rows")
    target = _aligned_target(target)
    _check_global_counts(global_counts)
    _check_flat(flat, packed)
    parr, tharr, barr, K = _step_consts(params, thetas, betas, kind)
    with _lib.on_device(x1.device):
        code = lib.nplda_train_step_grad_f32(_lib.ptr(x1), _lib.ptr(x2), x1.shape[0], ld, _lib.ptr(target),
                                             _lib.ptr(global_counts), parr, packed.D0, packed.D1, packed.D2, tharr, barr, K,
                                             float(alpha), kind, _lib.ptr(step), _lib.ptr(packed.buf), _lib.ptr(ws),
                                             ws.numel() * 4, _lib.ptr(flat), _lib.current_stream())
    _lib.check(code, "nplda_train_step_grad_f32")
    return flat


def train_step_grad_rows(table, rows1, rows2, target, params, thetas, betas, alpha, kind, step, packed, ws, flat,
                         global_counts=None):
    """nplda_train_step_grad_rows_f32: train_step_grad on the pairs (table[rows1], table[rows2]); the first kernel gathers
    the rows itself.  `ws`: train_step_workspace(B, packed, rows=True)."""
    lib = _lib.load()
    _need_fp32(packed, "train_step_grad_rows")
    table, ldt = _rows(table, "table", packed.D0)
    rows1, rows2, B = _index_rows(rows1, rows2, target, table.device)
    target = _aligned_target(target)
    _check_global_counts(global_counts)
    _check_flat(flat, packed)
    parr, tharr, barr, K = _step_consts(params, thetas, betas, kind)
    with _lib.on_device(table.device):
        code = lib.nplda_train_step_grad_rows_f32(_lib.ptr(table), table.shape[0], ldt, _lib.ptr(rows1), _lib.ptr(rows2), B,
                                                  _lib.ptr(target), _lib.ptr(global_counts), parr, packed.D0, packed.D1,
                                                  packed.D2, tharr, barr, K, float(alpha), kind, _lib.ptr(step),
                                                  _lib.ptr(packed.buf), _lib.ptr(ws), ws.numel() * 4, _lib.ptr(flat),
                                                  _lib.current_stream())
    _lib.check(code, "nplda_train_step_grad_rows_f32")
    return flat


def train_step_grad_dx(x1, x2, target, params, thetas, betas, alpha, kind, step, packed, ws, flat, dx1, dx2,
                       global_counts=None):
    """nplda_train_step_grad_dx_f32: train_step_grad that also writes dL/dx1, dL/dx2 (float32 or bfloat16, as x1 / x2) — the
    data-parallel form of train_step_dx's first half.  `ws`: train_step_dx_workspace."""
    lib = _lib.load()
    _need_fp32(packed, "train_step_grad_dx")
    B, bf = _dx_rows("train_step_grad_dx", packed, x1, x2, dx1, dx2, target)
    target = _aligned_target(target, strict="train_step_grad_dx")
    _check_global_counts(global_counts)
    _check_flat(flat, packed)
    parr, tharr, barr, K = _step_consts(params, thetas, betas, kind)
    with _lib.on_device(x1.device):
        code = lib.nplda_train_step_grad_dx_f32(x1.data_ptr(), x2.data_ptr(), B, x1.stride(0), bf, _lib.ptr(target),
                                                _lib.ptr(global_counts), parr, packed.D0, packed.D1, packed.D2, tharr, barr, K,
                                                float(alpha), kind, _lib.ptr(step), _lib.ptr(packed.buf), _lib.ptr(ws),
                                                ws.numel() * 4, _lib.ptr(flat), dx1.data_ptr(), dx2.data_ptr(), dx1.stride(0),
                                                _lib.current_stream())
    _lib.check(code, "nplda_train_step_grad_dx_f32")
    return flat


def train_step_apply(flat, params, thetas, betas, alpha, kind, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps,
                     weight_decay, packed, loss, loss_sum=None):
    """nplda_train_step_apply_f32: the update half of the data-parallel step from the all-reduced `flat`."""
    lib = _lib.load()
    _need_fp32(packed, "train_step_apply")
    parr, tharr, barr, K = _step_consts(params, thetas, betas, kind)
    with _lib.on_device(flat.device):
        code = lib.nplda_train_step_apply_f32(_lib.ptr(flat), parr, packed.D0, packed.D1, packed.D2, tharr, barr, K,
                                              float(alpha), kind, _lib.ptr(exp_avg), _lib.ptr(exp_avg_sq), _lib.ptr(step),
                                              *_floats(lr, beta1, beta2, eps, weight_decay), _lib.ptr(packed.buf),
                                              _lib.ptr(loss), _lib.ptr(loss_sum), _lib.current_stream())
    _lib.check(code, "nplda_train_step_apply_f32")
    return loss


def train_step_dx(x1, x2, target, params, thetas, betas, alpha, kind, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps,
                  weight_decay, packed, ws, loss, dx1, dx2, loss_sum=None):
    """nplda_train_step_dx_f32: train_step that also writes dL/dx1, dL/dx2 into `dx1`, `dx2` (B, D0).  x1 / x2 and dx1 / dx2
    are all float32 or all bfloat16 (the head's arithmetic is fp32 either way).  Four launches.  `ws`: a float32 tensor of
    nplda_train_step_dx_workspace_bytes (train_step_dx_workspace)."""
    lib = _lib.load()
    _need_fp32(packed, "train_step_dx")
    B, bf = _dx_rows("train_step_dx", packed, x1, x2, dx1, dx2, target)
    target = _aligned_target(target, strict="train_step_dx")
    _check_inplace_params(params, thetas, "train_step_dx")
    parr, tharr, barr, K = _step_consts(params, thetas, betas, kind)
    with _lib.on_device(x1.device):
        code = lib.nplda_train_step_dx_f32(_lib.ptr(x1), _lib.ptr(x2), B, x1.stride(0), bf, _lib.ptr(target), parr, packed.D0,
                                           packed.D1, packed.D2, tharr, barr, K, float(alpha), kind, _lib.ptr(exp_avg),
                                           _lib.ptr(exp_avg_sq), _lib.ptr(step), *_floats(lr, beta1, beta2, eps, weight_decay),
                                           _lib.ptr(packed.buf), _lib.ptr(ws), ws.numel() * 4, _lib.ptr(loss),
                                           _lib.ptr(loss_sum), None, _lib.ptr(dx1), _lib.ptr(dx2), dx1.stride(0),
                                           _lib.current_stream())
    _lib.check(code, "nplda_train_step_dx_f32")
    return loss


def train_step_dx_workspace(B, packed, bf16):
    """Workspace tensor for train_step_dx (None when the fused step does not cover this size / shape)."""
    n = _lib.load().nplda_train_step_dx_workspace_bytes(B, packed.D0, packed.D1, packed.D2, 1 if bf16 else 0)
    if n == 0:
        return None
    return torch.empty(n // 4, dtype=torch.float32, device=packed.buf.device)


def train_step_rows(table, rows1, rows2, target, params, thetas, betas, alpha, kind, exp_avg, exp_avg_sq, step, lr, beta1,
                    beta2, eps, weight_decay, packed, ws, loss, grad_out=None, loss_sum=None):
    """nplda_train_step_rows_f32: train_step on the pairs (table[rows1], table[rows2]) of a resident x-vector matrix; the
    first kernel gathers the rows itself.  rows1 / rows2: int64 device tensors with values in [0, len(table))."""
    lib = _lib.load()
    _need_fp32(packed, "train_step_rows")
    table, ldt = _rows(table, "table", packed.D0)
    rows1, rows2, B = _index_rows(rows1, rows2, target, table.device)
    target = _aligned_target(target)
    _check_inplace_params(params, thetas, "train_step")
    parr, tharr, barr, K = _step_consts(params, thetas, betas, kind)
    with _lib.on_device(table.device):
        code = lib.nplda_train_step_rows_f32(_lib.ptr(table), table.shape[0], ldt, _lib.ptr(rows1), _lib.ptr(rows2), B,
                                             _lib.ptr(target), parr, packed.D0, packed.D1, packed.D2, tharr, barr, K,
                                             float(alpha), kind, _lib.ptr(exp_avg), _lib.ptr(exp_avg_sq), _lib.ptr(step),
                                             *_floats(lr, beta1, beta2, eps, weight_decay), _lib.ptr(packed.buf), _lib.ptr(ws),
                                             ws.numel() * 4, _lib.ptr(loss), _lib.ptr(loss_sum), _lib.ptr(grad_out),
                                             _lib.current_stream())
    _lib.check(code, "nplda_train_step_rows_f32")
    return loss


def train_step_records(table, cursor, stage, B, params, thetas, betas, alpha, kind, exp_avg, exp_avg_sq, step, lr, beta1, beta2,
                       eps, weight_decay, packed, ws, loss, grad_out=None, loss_sum=None):
    """nplda_train_step_records_f32: train_step_rows on the record in `stage` (uint8 device tensor of 20 B bytes:
    [rows1 (B int64) | rows2 (B int64) | labels (B float32)]); the step's last kernel copies the epoch's next record there
    (cursor: int64 device tensor [address of record 0, next record to stage, record count])."""
    lib = _lib.load()
    _need_fp32(packed, "train_step_records")
    table, ldt = _rows(table, "table", packed.D0)
    if cursor.dtype != torch.int64 or cursor.device != table.device or cursor.numel() != 3 or not cursor.is_contiguous():
        raise TypeError("cursor must be a contiguous int64 tensor of 3 elements on the table's device")
    if stage.dtype != torch.uint8 or stage.device != table.device or stage.numel() != 20 * int(B) or not stage.is_contiguous():
        raise TypeError("stage must be a contiguous uint8 tensor of 20 B bytes on the table's device")
    _check_inplace_params(params, thetas, "train_step")
    parr, tharr, barr, K = _step_consts(params, thetas, betas, kind)
    with _lib.on_device(table.device):
        code = lib.nplda_train_step_records_f32(_lib.ptr(table), table.shape[0], ldt, _lib.ptr(cursor), _lib.ptr(stage), int(B),
                                                parr, packed.D0, packed.D1, packed.D2, tharr, barr, K, float(alpha), kind,
                                                _lib.ptr(exp_avg), _lib.ptr(exp_avg_sq), _lib.ptr(step),
                                                *_floats(lr, beta1, beta2, eps, weight_decay), _lib.ptr(packed.buf),
                                                _lib.ptr(ws), ws.numel() * 4, _lib.ptr(loss), _lib.ptr(loss_sum),
                                                _lib.ptr(grad_out), _lib.current_stream())
    _lib.check(code, "nplda_train_step_records_f32")
    return loss


# ---- indexed scoring / gather -------------------------------------------------------------------

def _idx(t, name, dev):
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(t)
    if t.dtype != torch.int64:
        t = t.long()
    if t.device != dev:
        t = t.to(dev, non_blocking=True)
    return t.contiguous()


def score_indexed(z, q, i1, i2, packed):
    """nplda_score_indexed_f32: z (N, ldz), q (N) from embed(); i1, i2 int64 (B) -> (B,) scores.  q=None: the self terms
    are formed from the z rows inside the kernel (sum_d Q_d z_d^2: two scattered 4-byte reads per pair less)."""
    lib = _lib.load()
    _need_fp32(packed, "score_indexed")
    _require_dev_f32(z, "z")
    if q is not None:
        _require_dev_f32(q, "q")
        q = q.contiguous()
    if z.dim() != 2 or z.stride(1) != 1 or z.stride(0) != packed.ldz or (q is not None and z.shape[0] != q.shape[0]):
        raise ValueError("z must be the (N, ldz) table returned by embed() and q its (N,) self terms")
    dev = z.device
    i1, i2 = _idx(i1, "i1", dev), _idx(i2, "i2", dev)
    if i1.shape != i2.shape or i1.dim() != 1:
        raise ValueError("i1 and i2 must be 1-D index tensors of the same length")
    B = i1.shape[0]
    s = torch.empty(B, dtype=torch.float32, device=dev)
    if B == 0:
        return s
    with _lib.on_device(dev):
        code = lib.nplda_score_indexed_f32(_lib.ptr(z), packed.ldz, _lib.ptr(q), z.shape[0], _lib.ptr(i1),
                                           _lib.ptr(i2), B, _lib.ptr(packed.buf), packed.D0, packed.D1, packed.D2,
                                           _lib.ptr(s), _lib.current_stream())
    _lib.check(code, "nplda_score_indexed_f32")
    return s


def score_embeddings(z1, z2, P_sqrt, Q):
    """nplda_score_embeddings_f32: forward_from_plda_embeddings on explicit (B, D2) tensors."""
    lib = _lib.load()
    for n, t in (("z1", z1), ("z2", z2), ("P_sqrt", P_sqrt), ("Q", Q)):
        _require_dev_f32(t, n)
    D2 = Q.numel()
    if z1.dim() != 2 or z1.shape != z2.shape or z1.shape[1] != D2:
        raise ValueError(f"z1, z2 must both be (B, {D2})")
    if z1.stride(1) != 1:
        z1 = z1.contiguous()
    if z2.stride(1) != 1:
        z2 = z2.contiguous()
    B = z1.shape[0]
    s = torch.empty(B, dtype=torch.float32, device=z1.device)
    if B == 0:
        return s
    ld1 = z1.stride(0) if B > 1 else D2
    ld2 = z2.stride(0) if B > 1 else D2
    with _lib.on_device(z1.device):
        code = lib.nplda_score_embeddings_f32(_lib.ptr(z1), ld1, _lib.ptr(z2), ld2, B, D2,
                                              _lib.ptr(P_sqrt.contiguous()), _lib.ptr(Q.contiguous()), _lib.ptr(s),
                                              _lib.current_stream())
    _lib.check(code, "nplda_score_embeddings_f32")
    return s


def gather_rows(table, idx, out=None):
    """nplda_gather_rows_f32: out[r] = table[idx[r]] for a resident (N, D0) float32 matrix.  `out`: an existing
    contiguous (B, D0) float32 device tensor to fill (static buffers of a captured step)."""
    lib = _lib.load()
    _require_dev_f32(table, "table")
    if table.dim() != 2 or table.stride(1) != 1 or table.stride(0) % 4 != 0 or table.shape[1] % 4 != 0:
        raise ValueError("table must be (N, D0) float32 with unit inner stride and D0 % 4 == 0")
    dev = table.device
    idx = _idx(idx, "idx", dev)
    B, D0 = idx.shape[0], table.shape[1]
    if out is None:
        out = torch.empty((B, D0), dtype=torch.float32, device=dev)
    else:
        _require_dev_f32(out, "out")
        if out.shape != (B, D0) or not out.is_contiguous() or out.device != dev:
            raise ValueError("out must be a contiguous (len(idx), D0) float32 tensor on the table's device")
    if B == 0:
        return out
    with _lib.on_device(dev):
        code = lib.nplda_gather_rows_f32(_lib.ptr(table), table.stride(0), table.shape[0], _lib.ptr(idx), B, D0,
                                         _lib.ptr(out), D0, _lib.current_stream())
    _lib.check(code, "nplda_gather_rows_f32")
    return out


_BAD_FLAGS = {}
KEYERROR_DEFERRED = False  # compat.install(lean=True): see gather_pairs_mapped


def _bad_flag(dev, stream=0):
    """The gather kernels' error word of a device: one int32 in PINNED host memory (the kernel ORs into it over the bus,
    only when a trial number is bad; the host reads it with a load, no copy) -> (tensor, its numpy view)."""
    hit = _BAD_FLAGS.get((dev, stream))  # (a word per stream: whose launch raised it is then unambiguous)
    if hit is None:
        t = torch.zeros(1, dtype=torch.int32).pin_memory()
        hit = _BAD_FLAGS[(dev, stream)] = (t, t.numpy())
    return hit


def _raise_bad(view):
    bad = int(view[0])
    if bad:
        view[0] = 0
        raise KeyError("trial index is outside num_to_id_dict" if bad & 1
                       else "trial index refers to an utterance that is not in mega_dict")


def check_trial_indices(device=None):
    """Wait for the gathers enqueued so far and raise the KeyError of any bad trial number among them (the deferred mode's
    explicit check: validate() and train() at the end of every epoch call it).  In deferred mode the step on a bad batch is
    NOT recoverable: its rows are NaN, so the loss, the gradients and — after the optimiser's step — every parameter are NaN
    by the time the KeyError surfaces; the error says which run to throw away, it does not save it."""
    synced = set()
    for (dev, _), (_, view) in list(_BAD_FLAGS.items()):
        if device is None or torch.device(device) == dev:
            if dev not in synced:
                torch.cuda.synchronize(dev)  # (every stream of the device: a word per stream)
                synced.add(dev)
            _raise_bad(view)


def gather_pairs_mapped(table, num_map, num1, num2, deferred=None):
    """nplda_gather_pairs_mapped_f32: (table[num_map[num1]], table[num_map[num2]]) as two (B, D0) float32 tensors in ONE
    launch — load_xvec_trials_from_numbatch on the device.  Raises the reference's KeyError when a number is outside the
    map or names an utterance that is not in the table: the kernel raises a word in pinned host memory, read after a
    stream synchronise (no copy).  deferred=True (default: KEYERROR_DEFERRED) skips that synchronise — the host keeps
    running ahead of the device — and raises for the launches that HAVE finished: the KeyError of a bad batch then surfaces
    at the next call (or at check_trial_indices()), its rows being NaN in the meantime."""
    lib = _lib.load()
    _require_dev_f32(table, "table")
    if table.dim() != 2 or table.stride(1) != 1 or table.stride(0) % 4 != 0 or table.shape[1] % 4 != 0:
        raise ValueError("table must be (N, D0) float32 with unit inner stride and D0 % 4 == 0")
    dev = table.device
    num1, num2 = _idx(num1.reshape(-1), "num1", dev), _idx(num2.reshape(-1), "num2", dev)
    if num1.shape != num2.shape:
        raise ValueError("num1 and num2 must have the same length")
    if num_map.dtype != torch.int64 or num_map.device != dev or not num_map.is_contiguous():
        raise ValueError("num_map must be a contiguous int64 tensor on the table's device")
    B, D0 = num1.shape[0], table.shape[1]
    out = torch.empty((2, B, D0), dtype=torch.float32, device=dev)
    if B == 0:
        return out[0], out[1]
    if deferred is None:
        deferred = KEYERROR_DEFERRED
    with _lib.on_device(dev):  # (the launch goes to the CURRENT device: dev may not be it in a multi-GPU process)
        st = _lib.current_stream(dev)
        flag, view = _bad_flag(dev, st)
        if deferred:
            _raise_bad(view)  # (an earlier batch's)
        code = lib.nplda_gather_pairs_mapped_f32(table.data_ptr(), table.stride(0), table.shape[0], num_map.data_ptr(),
                                                 num_map.numel(), num1.data_ptr(), num2.data_ptr(), B, D0, out[0].data_ptr(),
                                                 out[1].data_ptr(), D0, flag.data_ptr(), st)
        _lib.check(code, "nplda_gather_pairs_mapped_f32")
        if not deferred:
            torch.cuda.current_stream(dev).synchronize()
    if not deferred:
        _raise_bad(view)
    return out[0], out[1]


# ---- adaptive score normalisation -----------------------------------------------------------------

class PreparedCohort:
    """What nplda_cohort_stats_f32 derives from the cohort alone (nplda_cohort_prepare_f32), kept for the calls that follow:
    `state` is None when the shape takes the spilling path (nothing to prepare)."""
    __slots__ = ("state", "M", "topn", "ldz", "key")

    def __init__(self, state, M, topn, ldz, key):
        self.state, self.M, self.topn, self.ldz, self.key = state, M, topn, ldz, key


def _cohort_key(z_coh, q_coh, packed):
    """What a PreparedCohort was derived from: the cohort's embedding tables and the packed model image (addresses +
    in-place versions).  cohort_stats(prepared=...) recomputes it: a state prepared for ANOTHER cohort or model of the same
    size would otherwise feed its first moments and covariance image into this call's row means and thresholds."""
    def ver(t):
        return 0 if t.is_inference() else t._version
    return (z_coh.data_ptr(), ver(z_coh), q_coh.data_ptr(), ver(q_coh), packed.buf.data_ptr(), ver(packed.buf))


def cohort_prepare(z_coh, q_coh, packed, topn=500):
    """nplda_cohort_prepare_f32: the cohort-only part of cohort_stats (Gram matrix, first moments, the covariance image the
    row thresholds are proposed from), once per (model, cohort, top-N) -> PreparedCohort for cohort_stats(prepared=...)."""
    lib = _lib.load()
    _need_fp32(packed, "cohort_prepare")
    _require_dev_f32(z_coh, "z_coh")
    _require_dev_f32(q_coh, "q_coh")
    if z_coh.stride(0) != packed.ldz:
        raise ValueError("z_coh must come from embed() (row stride = packed.ldz)")
    M = z_coh.shape[0]
    key = _cohort_key(z_coh, q_coh, packed)
    nb = lib.nplda_cohort_state_bytes(M, int(topn), packed.D1, packed.D2) if M > 0 else 0
    if nb == 0:
        return PreparedCohort(None, M, int(topn), packed.ldz, key)
    state = torch.empty((nb + 255) // 4 + 64, dtype=torch.float32, device=z_coh.device)
    off = (-state.data_ptr()) % 256 // 4
    state = state[off:off + (nb + 3) // 4]  # 256-byte aligned view
    qc = q_coh.contiguous()
    with _lib.on_device(z_coh.device):
        code = lib.nplda_cohort_prepare_f32(_lib.ptr(z_coh), _lib.ptr(qc), M, packed.ldz, _lib.ptr(packed.buf), packed.D0,
                                            packed.D1, packed.D2, int(topn), _lib.ptr(state), nb, _lib.current_stream())
    _lib.check(code, "nplda_cohort_prepare_f32")
    return PreparedCohort(state, M, int(topn), packed.ldz, key)


def cohort_stats(z_rows, q_rows, z_coh, q_coh, packed, topn=500, select="lowest", max_ws_bytes=None, force_spill=False,
                 return_fallback_rows=False, prepared=None):
    """nplda_cohort_stats_f32: (R, 4) float64 rows of (mean, std, mean_top, std_top).  force_spill (tests / A-B timing):
    hand the call a workspace just below the fused path's minimum, so that it materialises the score matrix.
    return_fallback_rows (diagnostics): also return how many rows of the (last chunk of the) fused path were handed to the
    general path because the proposed threshold did not bracket their N-th smallest score (reads the workspace: a sync)."""
    lib = _lib.load()
    _need_fp32(packed, "cohort_stats")
    for n, t in (("z_rows", z_rows), ("q_rows", q_rows), ("z_coh", z_coh), ("q_coh", q_coh)):
        _require_dev_f32(t, n)
    if z_rows.stride(0) != packed.ldz or z_coh.stride(0) != packed.ldz:
        raise ValueError("z tables must come from embed() (row stride = packed.ldz)")
    if select not in ("lowest", "highest"):
        raise ValueError("select must be 'lowest' (reference semantics) or 'highest'")
    R, M = z_rows.shape[0], z_coh.shape[0]
    dev = z_rows.device
    stats = torch.empty((R, 4), dtype=torch.float64, device=dev)
    if R == 0:
        return stats
    wsb = lib.nplda_cohort_workspace_bytes_ex(R, M, int(topn), packed.D1, packed.D2)
    if force_spill:
        wsb = lib.nplda_cohort_workspace_bytes(R, M)
    if max_ws_bytes is not None:
        # never below one score row, nor below what keeps the call on the path its shape selects (fused / spilling)
        floor = max(256 + ((M + 3) // 4 * 4) * 4,
                    lib.nplda_cohort_fused_min_workspace_bytes(M, int(topn), packed.D1, packed.D2))
        wsb = max(min(wsb, int(max_ws_bytes)), floor)
    if force_spill:
        fmin = lib.nplda_cohort_fused_min_workspace_bytes(M, int(topn), packed.D1, packed.D2)
        if fmin:
            wsb = min(wsb, fmin - 256)
            if wsb < 256 + ((M + 3) // 4 * 4) * 4:
                raise ValueError("no workspace size selects the spilling path for this shape")
    ws = torch.empty(wsb // 4, dtype=torch.float32, device=dev)
    use_prep = prepared is not None and prepared.state is not None and not force_spill
    if prepared is not None and (prepared.M != M or prepared.topn != int(topn) or prepared.ldz != packed.ldz):
        raise ValueError("prepared cohort does not belong to this cohort table / top-N")
    if use_prep and prepared.key != _cohort_key(z_coh, q_coh, packed):  # (state None: nothing was derived, nothing to mismatch)
        raise ValueError("prepared cohort was derived from other cohort tables / another model image (or they were "
                         "modified since): call cohort_prepare() again")
    with _lib.on_device(dev):
        if use_prep:
            st = prepared.state
            code = lib.nplda_cohort_stats_prepared_f32(
                _lib.ptr(z_rows), _lib.ptr(q_rows.contiguous()), R, _lib.ptr(z_coh), _lib.ptr(q_coh.contiguous()), M, packed.ldz,
                _lib.ptr(packed.buf), packed.D0, packed.D1, packed.D2, int(topn), 1 if select == "lowest" else 0, _lib.ptr(stats),
                _lib.ptr(ws), wsb, _lib.ptr(st), st.numel() * 4, _lib.current_stream())
        else:
            code = lib.nplda_cohort_stats_f32(_lib.ptr(z_rows), _lib.ptr(q_rows.contiguous()), R, _lib.ptr(z_coh),
                                              _lib.ptr(q_coh.contiguous()), M, packed.ldz, _lib.ptr(packed.buf), packed.D0,
                                              packed.D1, packed.D2, int(topn), 1 if select == "lowest" else 0,
                                              _lib.ptr(stats), _lib.ptr(ws), wsb, _lib.current_stream())
    _lib.check(code, "nplda_cohort_stats_prepared_f32" if use_prep else "nplda_cohort_stats_f32")
    if return_fallback_rows:
        fused = lib.nplda_cohort_fused_min_workspace_bytes(M, int(topn), packed.D1, packed.D2)
        # word 8 of a fused workspace: the fail count (kFusedFailWord, csrc/nplda_cohort_fused.h)
        return stats, (int(ws.view(torch.int32)[8].item()) if fused and wsb >= fused else None)
    return stats


def cohort_scores(z_rows, q_rows, z_coh, q_coh, packed):
    """The (R, M) float32 cohort score matrix S = q_r + q_m + 2 (z_r * P) z_m^T as the spilling path of
    nplda_cohort_stats_f32 writes it (diagnostics and tests; the reference reads this table from a file).  The call asks
    for top-N = M, which no shape's fused plan accepts, and brings a workspace of exactly the control block + R score rows:
    one chunk, whose rows are returned as a view of the workspace (row stride M rounded up to 4).  A matrix above 4 GiB is
    walked in row chunks and copied out."""
    lib = _lib.load()
    _need_fp32(packed, "cohort_scores")
    for n, t in (("z_rows", z_rows), ("q_rows", q_rows), ("z_coh", z_coh), ("q_coh", q_coh)):
        _require_dev_f32(t, n)
    if z_rows.stride(0) != packed.ldz or z_coh.stride(0) != packed.ldz:
        raise ValueError("z tables must come from embed() (row stride = packed.ldz)")
    R, M = z_rows.shape[0], z_coh.shape[0]
    dev = z_rows.device
    if R == 0 or M == 0:
        return torch.empty((R, M), dtype=torch.float32, device=dev)
    lds = (M + 3) // 4 * 4
    ctl = 64  # floats of the control block in front of the score rows (kCohortCtlBytes, csrc/nplda_cohort.hip)
    rows_per = max(1, min(R, (4 << 30) // (lds * 4)))
    q_rows, q_coh = q_rows.contiguous(), q_coh.contiguous()
    stats = torch.empty((rows_per, 4), dtype=torch.float64, device=dev)
    out = None if rows_per == R else torch.empty((R, M), dtype=torch.float32, device=dev)
    for r0 in range(0, R, rows_per):
        rc = min(rows_per, R - r0)
        ws = torch.empty(ctl + rc * lds, dtype=torch.float32, device=dev)
        with _lib.on_device(dev):
            code = lib.nplda_cohort_stats_f32(_lib.ptr(z_rows[r0:r0 + rc]), _lib.ptr(q_rows[r0:r0 + rc]), rc, _lib.ptr(z_coh),
                                              _lib.ptr(q_coh), M, packed.ldz, _lib.ptr(packed.buf), packed.D0, packed.D1,
                                              packed.D2, M, 1, _lib.ptr(stats), _lib.ptr(ws), ws.numel() * 4,
                                              _lib.current_stream())
        _lib.check(code, "nplda_cohort_stats_f32")
        S = ws[ctl:].view(rc, lds)[:, :M]
        if out is None:
            return S
        out[r0:r0 + rc] = S
    return out


TOPK_MAX_K = 128  # NPLDA_TOPK_MAX_K, include/nplda_hip.h
_TOPK_MASKS = {None: 0, "different": 1, "same": 2}


def topk_scores(z_rows, q_rows, z_tab, q_tab, packed, k, largest=True, labels=None, mask=None, groups=None, self_rows=None):
    """nplda_topk_scores_f32: for each of the R rows the k best-scoring of the M table rows -> (vals (R, k) float32,
    idx (R, k) int64), best first, equal scores in ascending column order; slots a row has no eligible column for hold
    -1 and -inf (largest) / +inf (smallest).  The z tables and q vectors come from embed().  mask: None, "different" or "same"
    with labels = (row labels (R,), table labels (M,)); groups = (row groups, table groups) restricts a row to the columns of
    its group; self_rows (R,) int64 names the table row each row IS, which is then never returned for it.  The R x M score
    matrix is never materialised."""
    lib = _lib.load()
    _need_fp32(packed, "topk_scores")
    for n, t in (("z_rows", z_rows), ("q_rows", q_rows), ("z_tab", z_tab), ("q_tab", q_tab)):
        _require_dev_f32(t, n)
    for n, t in (("z_rows", z_rows), ("z_tab", z_tab)):
        if t.dim() != 2 or t.shape[1] != packed.ldz or (t.shape[0] > 1 and t.stride(0) != packed.ldz) or t.stride(1) != 1:
            raise ValueError(f"{n} must come from embed() (shape (rows, {packed.ldz}), row stride = packed.ldz)")
    R, M, dev = z_rows.shape[0], z_tab.shape[0], z_rows.device
    if q_rows.shape != (R,) or q_tab.shape != (M,):
        raise ValueError("q_rows / q_tab must hold one self term per row of z_rows / z_tab")
    if z_tab.device != dev or packed.device != dev:
        raise ValueError("z_rows, z_tab and the packed model must live on one device")
    k = int(k)
    if not 1 <= k <= TOPK_MAX_K:
        raise ValueError(f"k must be in 1 .. {TOPK_MAX_K} (got {k})")
    if mask not in _TOPK_MASKS:
        raise ValueError("mask must be None, 'different' or 'same'")
    lab_r = lab_t = grp_r = grp_t = None
    if mask is not None:
        if labels is None or len(labels) != 2:
            raise ValueError("mask needs labels = (row labels, table labels)")
        lab_r, lab_t = _labels(labels[0], "labels[0]", R, dev), _labels(labels[1], "labels[1]", M, dev)
    if groups is not None:
        if len(groups) != 2:
            raise ValueError("groups = (row groups, table groups)")
        grp_r, grp_t = _labels(groups[0], "groups[0]", R, dev), _labels(groups[1], "groups[1]", M, dev)
    if self_rows is not None:
        self_rows = _idx(self_rows, "self_rows", dev)
        if self_rows.shape != (R,):
            raise ValueError("self_rows must name one table row per row of z_rows")
    vals = torch.empty((R, k), dtype=torch.float32, device=dev)
    idx = torch.empty((R, k), dtype=torch.int64, device=dev)
    if R == 0:
        return vals, idx
    wsb = lib.nplda_topk_workspace_bytes(R, M, packed.D2, k)
    if wsb == 0:
        raise _lib.NpldaHipError(f"topk_scores: R = {R}, M = {M}, D2 = {packed.D2}, k = {k} is outside the compiled kernel set")
    ws = torch.empty(wsb // 4, dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        code = lib.nplda_topk_scores_f32(_lib.ptr(z_rows), _lib.ptr(q_rows.contiguous()), R, _lib.ptr(z_tab),
                                         _lib.ptr(q_tab.contiguous()), M, packed.ldz, _lib.ptr(packed.buf), packed.D0, packed.D1,
                                         packed.D2, k, 1 if largest else 0, _TOPK_MASKS[mask], _lib.ptr(lab_r), _lib.ptr(lab_t),
                                         _lib.ptr(grp_r), _lib.ptr(grp_t), _lib.ptr(self_rows), _lib.ptr(vals), _lib.ptr(idx),
                                         _lib.ptr(ws), wsb, _lib.current_stream())
    _lib.check(code, "nplda_topk_scores_f32")
    return vals, idx


AHC_LINKAGES = {"average": 0, "complete": 1, "single": 2}  # NPLDA_AHC_*, include/nplda_hip.h
# nplda_ahc_merge as a numpy record (24 bytes)
AHC_MERGE_DTYPE = [("a", "<i4"), ("b", "<i4"), ("value", "<f8"), ("size_after", "<i4"), ("reserved", "<i4")]


class RaggedOffsets:
    """The row offsets of P independent problems over one table, on the host (int64 numpy, what the C entry points check and
    size their launches by) and on a device (what the kernels read).  Make one outside a graph capture: building it copies
    from the host.  max_rows: the most rows a problem may have (None: nplda_ahc_max_n(), what the clustering and the VB-HMM
    take; ops.der lays its frames and turns out with larger ones)."""

    __slots__ = ("host", "dev", "P", "rows", "elems", "records")

    def __init__(self, offsets, device, max_rows=None):
        import numpy as np
        host = np.ascontiguousarray(np.asarray(offsets.cpu() if isinstance(offsets, torch.Tensor) else offsets, dtype=np.int64))
        if host.ndim != 1 or host.size < 1 or host[0] != 0 or (np.diff(host) < 0).any():
            raise ValueError("offsets must be P + 1 non-decreasing row offsets that start at 0")
        lib = _lib.load()
        self.host, self.P, self.rows = host, host.size - 1, int(host[-1])
        if max_rows is not None:
            if self.P and int(np.diff(host).max()) > int(max_rows):
                raise ValueError(f"a problem may have at most {int(max_rows)} rows")
        elif self.P and int(np.diff(host).max()) > lib.nplda_ahc_max_n():
            raise ValueError(f"a problem may have at most {lib.nplda_ahc_max_n()} rows")
        n = np.diff(host)
        self.elems, self.records = int((n * n).sum()), int(np.maximum(n - 1, 0).sum())
        self.dev = torch.from_numpy(host).to(device)

    @property
    def hptr(self):
        return self.host.ctypes.data


def _ragged(offsets, rows, dev):
    if offsets is None:
        offsets = [0, rows]
    if not isinstance(offsets, RaggedOffsets):
        offsets = RaggedOffsets(offsets, dev)
    if offsets.dev.device != dev:
        raise ValueError("the offsets live on another device")
    return offsets


def score_matrix(z, q, packed, offsets=None):
    """nplda_score_matrix_f32: the dense score matrix of every problem's rows against themselves, exactly symmetric with a
    +0.0 diagonal; for i < j the bits of topk_scores (row i, column j).  z, q come from embed(); offsets: P + 1 row offsets
    (a sequence or a RaggedOffsets) -> the matrices one after the other in a flat float32 tensor (problem p's n_p x n_p at
    element sum n_r^2 of the problems before it); None: the whole table is one problem -> (N, N)."""
    lib = _lib.load()
    _need_fp32(packed, "score_matrix")
    _require_dev_f32(z, "z")
    _require_dev_f32(q, "q")
    if z.dim() != 2 or z.shape[1] != packed.ldz or (z.shape[0] > 1 and z.stride(0) != packed.ldz) or z.stride(1) != 1:
        raise ValueError(f"z must come from embed() (shape (rows, {packed.ldz}), row stride = packed.ldz)")
    N, dev = z.shape[0], z.device
    if q.shape != (N,) or packed.device != dev:
        raise ValueError("q must hold one self term per row of z, on the device of z and the packed model")
    single = offsets is None
    offs = _ragged(offsets, N, dev)
    if offs.rows != N:
        raise ValueError(f"the offsets cover {offs.rows} rows, z has {N}")
    out = torch.empty(offs.elems, dtype=torch.float32, device=dev)
    if offs.elems:
        with _lib.on_device(dev):
            code = lib.nplda_score_matrix_f32(_lib.ptr(z), packed.ldz, _lib.ptr(q.contiguous()), offs.hptr, _lib.ptr(offs.dev),
                                              offs.P, _lib.ptr(packed.buf), packed.D0, packed.D1, packed.D2, _lib.ptr(out),
                                              _lib.current_stream())
        _lib.check(code, "nplda_score_matrix_f32")
    return out.view(N, N) if single else out


def ahc(S, offsets=None, linkage="average", threshold=float("-inf"), min_clusters=1):
    """nplda_ahc_f32: agglomerative clustering of every problem under its float32 score matrix in S (the layout of
    score_matrix; only the strict upper triangle is read) -> (merges, n_merges (P,), n_clusters (P,), labels (rows,)), all on
    the device.  merges is a uint8 tensor (records, 24): view its host copy with AHC_MERGE_DTYPE.  Each step merges the pair
    with the LARGEST linkage value (lowest (a, b) among equal ones); it stops before the first value < threshold or at
    min_clusters clusters."""
    lib = _lib.load()
    _require_dev_f32(S, "S")
    if linkage not in AHC_LINKAGES:
        raise ValueError(f"linkage must be one of {sorted(AHC_LINKAGES)}")
    threshold, min_clusters = float(threshold), int(min_clusters)
    if threshold != threshold or min_clusters < 1:
        raise ValueError("threshold must not be NaN and min_clusters must be at least 1")
    if not S.is_contiguous():
        S = S.contiguous()
    dev = S.device
    if offsets is None:
        if S.dim() != 2 or S.shape[0] != S.shape[1]:
            raise ValueError("without offsets S must be one square matrix")
        offsets = [0, S.shape[0]]
    offs = _ragged(offsets, 0, dev)
    if S.numel() != offs.elems:
        raise ValueError(f"S holds {S.numel()} scores, the offsets ask for {offs.elems}")
    merges = torch.empty((offs.records, 24), dtype=torch.uint8, device=dev)
    n_merges = torch.empty(offs.P, dtype=torch.int32, device=dev)
    n_clusters = torch.empty(offs.P, dtype=torch.int32, device=dev)
    labels = torch.empty(offs.rows, dtype=torch.int32, device=dev)
    if offs.P == 0:
        return merges, n_merges, n_clusters, labels
    wsb = lib.nplda_ahc_workspace_bytes(offs.hptr, offs.P)
    if wsb == 0:
        raise _lib.NpldaHipError("ahc: the offsets are outside what the kernel takes")
    ws = torch.empty(wsb // 8 if offs.records else 2, dtype=torch.float64, device=dev)
    with _lib.on_device(dev):
        code = lib.nplda_ahc_f32(_lib.ptr(S), offs.hptr, _lib.ptr(offs.dev), offs.P, AHC_LINKAGES[linkage], threshold,
                                 min_clusters, _lib.ptr(merges), _lib.ptr(n_merges), _lib.ptr(n_clusters), _lib.ptr(labels),
                                 _lib.ptr(ws), ws.numel() * 8, _lib.current_stream())
    _lib.check(code, "nplda_ahc_f32")
    return merges, n_merges, n_clusters, labels


SPECTRAL_NEIGHBOURS = (2, 3, 4, 6, 8, 12, 16, 24, 32, 48)  # the default candidate ladder (design/k25_spectral.md)


class SpectralResult:
    """What spectral() wrote, all on the device: per cell `eigenvalues` (P, C, max_clusters + 2), `kstar`, `n_sweeps`,
    `converged` (P, C) int32 and `ratio` (P, C) float64; per problem `chosen`, `n_clusters`, `n_kmeans_iters` (P,) int32;
    `labels` (rows,) int32; and, where asked for, `embedding` (rows, max_clusters) float64 (problem p's n x k matrix compact
    at row offsets[p]: see embedding_of), `degrees` (flat, cell (p, c) at offsets[p] C + c n_p) and `vectors` (flat, see
    vectors_of)."""

    __slots__ = ("eigenvalues", "kstar", "ratio", "n_sweeps", "converged", "chosen", "n_clusters", "n_kmeans_iters", "labels",
                 "embedding", "degrees", "vectors", "offsets", "neighbours", "max_clusters")

    def k_of(self, p):
        """Columns of problem p's embedding: min(k* of the chosen cell, n_p) (reads two words back)."""
        n = int(self.offsets[p + 1] - self.offsets[p])
        return min(int(self.kstar[p, int(self.chosen[p])]), n)

    def embedding_of(self, p):
        """Problem p's (n_p, k) embedding (a view)."""
        r0, n, k = int(self.offsets[p]), int(self.offsets[p + 1] - self.offsets[p]), self.k_of(p)
        return self.embedding.view(-1)[r0 * self.max_clusters:r0 * self.max_clusters + n * k].view(n, k)

    def degrees_of(self, p, c):
        r0, n, C = int(self.offsets[p]), int(self.offsets[p + 1] - self.offsets[p]), len(self.neighbours)
        return self.degrees[r0 * C + c * n:r0 * C + (c + 1) * n]

    def vectors_of(self, p, c):
        """Cell (p, c)'s eigenvectors as ROWS, (min(max_clusters + 1, n_p), n_p), in eigenvalue order (a view)."""
        import numpy as np
        n = np.diff(self.offsets)
        rows = np.minimum(self.max_clusters + 1, n)
        C = len(self.neighbours)
        base = int((C * rows[:p] * n[:p]).sum()) + c * int(rows[p] * n[p])
        return self.vectors[base:base + int(rows[p] * n[p])].view(int(rows[p]), int(n[p]))


def _spectral_table(neighbours, lib):
    import numpy as np
    nb = np.atleast_1d(np.asarray(neighbours))
    if nb.ndim != 1 or nb.dtype.kind not in "iu" or not 1 <= nb.size <= lib.nplda_spectral_max_candidates() or \
            (nb < 1).any() or (nb >= 2 ** 31).any() or (np.diff(nb) <= 0).any():
        raise ValueError(f"neighbours must be 1 .. {lib.nplda_spectral_max_candidates()} positive, strictly increasing integers")
    return np.ascontiguousarray(nb.astype(np.int32))


def spectral_workspace_bytes(offsets, n_candidates):
    """nplda_spectral_workspace_bytes for host offsets (any sequence) and a candidate count; 0 where they are not acceptable."""
    import numpy as np
    host = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64))
    return int(_lib.load().nplda_spectral_workspace_bytes(host.ctypes.data, host.size - 1, int(n_candidates)))


def spectral(S, offsets=None, neighbours=SPECTRAL_NEIGHBOURS, min_clusters=1, max_clusters=None, max_iters=100,
             return_embedding=False, return_degrees=False, return_vectors=False):
    """nplda_spectral_f32: spectral clustering of every problem under its float32 score matrix in S (the layout of
    score_matrix) with the neighbour count chosen per problem among `neighbours` by the normalised maximum eigengap
    (include/nplda_hip.h has the definitions) -> SpectralResult.  max_clusters None: nplda_spectral_max_k().  Nothing is read
    back: a cell whose eigensolver stopped at its sweep limit has converged == 0 (cluster.spectral_cluster raises on it)."""
    lib = _lib.load()
    _require_dev_f32(S, "S")
    nb = _spectral_table(neighbours, lib)
    limit = int(lib.nplda_spectral_max_k())
    min_clusters, max_iters = int(min_clusters), int(max_iters)
    max_clusters = limit if max_clusters is None else int(max_clusters)
    if min_clusters < 1 or not min_clusters <= max_clusters <= limit or max_iters < 1:
        raise ValueError(f"need 1 <= min_clusters <= max_clusters <= {limit} and max_iters >= 1")
    if not S.is_contiguous():
        S = S.contiguous()
    dev = S.device
    if offsets is None:
        if S.dim() != 2 or S.shape[0] != S.shape[1]:
            raise ValueError("without offsets S must be one square matrix")
        offsets = [0, S.shape[0]]
    offs = _ragged(offsets, 0, dev)
    if S.numel() != offs.elems:
        raise ValueError(f"S holds {S.numel()} scores, the offsets ask for {offs.elems}")
    if offs.P and int((offs.host[1:] - offs.host[:-1]).max()) > lib.nplda_spectral_max_n():
        raise ValueError(f"a problem may have at most {lib.nplda_spectral_max_n()} rows")
    import numpy as np
    P, C, n = offs.P, int(nb.size), offs.host[1:] - offs.host[:-1]
    out = SpectralResult()
    out.offsets, out.neighbours, out.max_clusters = offs.host, nb, max_clusters
    out.eigenvalues = torch.empty((P, C, max_clusters + 2), dtype=torch.float64, device=dev)
    out.ratio = torch.empty((P, C), dtype=torch.float64, device=dev)
    out.kstar, out.n_sweeps, out.converged = (torch.empty((P, C), dtype=torch.int32, device=dev) for _ in range(3))
    out.chosen, out.n_clusters, out.n_kmeans_iters = (torch.empty(P, dtype=torch.int32, device=dev) for _ in range(3))
    out.labels = torch.empty(offs.rows, dtype=torch.int32, device=dev)
    out.embedding = torch.empty((offs.rows, max_clusters), dtype=torch.float64, device=dev) if return_embedding else None
    out.degrees = torch.empty(offs.rows * C, dtype=torch.float64, device=dev) if return_degrees else None
    out.vectors = torch.empty(int((C * np.minimum(max_clusters + 1, n) * n).sum()), dtype=torch.float64, device=dev) \
        if return_vectors else None
    if P == 0:
        return out
    wsb = lib.nplda_spectral_workspace_bytes(offs.hptr, P, C)
    if wsb == 0:
        raise _lib.NpldaHipError("spectral: the offsets are outside what the kernel takes")
    ws = torch.empty(wsb // 8 if offs.rows else 2, dtype=torch.float64, device=dev)
    with _lib.on_device(dev):
        code = lib.nplda_spectral_f32(_lib.ptr(S), offs.hptr, _lib.ptr(offs.dev), P, nb.ctypes.data, C, min_clusters,
                                      max_clusters, max_iters, _lib.ptr(out.eigenvalues), _lib.ptr(out.kstar),
                                      _lib.ptr(out.ratio), _lib.ptr(out.n_sweeps), _lib.ptr(out.converged), _lib.ptr(out.chosen),
                                      _lib.ptr(out.n_clusters), _lib.ptr(out.n_kmeans_iters), _lib.ptr(out.labels),
                                      _lib.ptr(out.embedding), _lib.ptr(out.degrees), _lib.ptr(out.vectors), _lib.ptr(ws),
                                      ws.numel() * 8, _lib.current_stream())
    _lib.check(code, "nplda_spectral_f32")
    return out


def spectral_kmeans(E, offsets=None, k=2, max_iters=100):
    """nplda_spectral_kmeans_f64: the k-means of spectral() on caller-given rows.  E: (rows, dim) float64 on the device, each
    problem's rows partitioned into min(k, n_p) clusters -> (labels (rows,), n_clusters (P,), n_iters (P,)), int32 on the
    device."""
    lib = _lib.load()
    if not isinstance(E, torch.Tensor) or not E.is_cuda or E.dtype != torch.float64 or E.dim() != 2:
        raise TypeError("E must be a (rows, dim) float64 tensor on a HIP device")
    limit = int(lib.nplda_spectral_max_k())
    k, max_iters = int(k), int(max_iters)
    if not 1 <= E.shape[1] <= limit or not 1 <= k <= limit or max_iters < 1:
        raise ValueError(f"need 1 <= dim <= {limit}, 1 <= k <= {limit} and max_iters >= 1")
    E = E.contiguous()
    dev, rows, dim = E.device, E.shape[0], E.shape[1]
    offs = _ragged(offsets, rows, dev)
    if offs.rows != rows:
        raise ValueError(f"the offsets cover {offs.rows} rows, E has {rows}")
    if offs.P and int((offs.host[1:] - offs.host[:-1]).max()) > lib.nplda_spectral_max_n():
        raise ValueError(f"a problem may have at most {lib.nplda_spectral_max_n()} rows")
    labels = torch.empty(rows, dtype=torch.int32, device=dev)
    n_clusters = torch.empty(offs.P, dtype=torch.int32, device=dev)
    n_iters = torch.empty(offs.P, dtype=torch.int32, device=dev)
    if offs.P == 0:
        return labels, n_clusters, n_iters
    wsb = lib.nplda_spectral_kmeans_workspace_bytes(offs.hptr, offs.P)
    ws = torch.empty(max(wsb // 8, 2), dtype=torch.float64, device=dev)
    with _lib.on_device(dev):
        code = lib.nplda_spectral_kmeans_f64(_lib.ptr(E), offs.hptr, _lib.ptr(offs.dev), offs.P, dim, k, max_iters,
                                             _lib.ptr(n_clusters), _lib.ptr(n_iters), _lib.ptr(labels), _lib.ptr(ws),
                                             ws.numel() * 8, _lib.current_stream())
    _lib.check(code, "nplda_spectral_kmeans_f64")
    return labels, n_clusters, n_iters


def vbhmm(z, offsets, spk_offsets, psi, labels_init=None, gamma_init=None, pi_init=None, Fa=0.3, Fb=17.0, loop_prob=0.99,
          epsilon=1e-4, init_smoothing=5.0, max_iters=40):
    """nplda_vbhmm_f64: VB-HMM resegmentation (VBx) of P problems over one table, all in float64 on the device.  z: (rows, ld)
    float32 embeddings as embed() wrote them (ld a multiple of 4), problem p's rows offsets[p] .. offsets[p + 1] IN TIME
    ORDER; spk_offsets: P + 1 offsets of the problems' speaker slots (S_p each, at most nplda_vbhmm_max_speakers());
    offsets, spk_offsets: sequences or RaggedOffsets (offsets None: the whole table is one problem);
    psi: (D2,) between-class variances, D2 <= ld.  Exactly one of labels_init ((rows,) integer labels local to the problem;
    one outside 0 .. S_p - 1 gives the uniform row) and gamma_init (flat float64, the T_p x S_p blocks one after the other).
    -> (gamma (sum T_p S_p,), pi (sum S_p,), elbo (P, max_iters) with NaN where not executed, n_iters (P,), labels (rows,),
    n_speakers (P,)), all on the device."""
    lib = _lib.load()
    _require_dev_f32(z, "z")
    if z.dim() != 2 or z.stride(1) != 1 or (z.shape[0] > 1 and z.stride(0) % 4) or z.data_ptr() % 16:
        raise ValueError("z must be (rows, ld) float32 with unit column stride, a row stride that is a multiple of 4 and a "
                         "16-byte aligned start: what embed() returns")
    rows, dev = z.shape[0], z.device
    ldz = z.stride(0) if rows > 1 else max(z.shape[1] + 3 & ~3, 4)
    psi = torch.as_tensor(psi)
    if psi.dim() != 1 or not 1 <= psi.shape[0] <= z.shape[1]:
        raise ValueError(f"psi must be (D2,) with 1 <= D2 <= {z.shape[1]}, got {tuple(psi.shape)}")
    D2 = int(psi.shape[0])
    psi = psi.detach().to(device=dev, dtype=torch.float64).contiguous()
    Fa, Fb, loop_prob, epsilon, init_smoothing = float(Fa), float(Fb), float(loop_prob), float(epsilon), float(init_smoothing)
    max_iters = int(max_iters)
    if not (0.0 < Fa < float("inf") and 0.0 < Fb < float("inf")) or not 0.0 <= loop_prob < 1.0:
        raise ValueError("Fa and Fb must be positive and finite, loop_prob in [0, 1)")
    if epsilon != epsilon or not init_smoothing >= 0.0 or not 1 <= max_iters <= lib.nplda_vbhmm_max_iters():
        raise ValueError(f"epsilon must not be NaN, init_smoothing >= 0, max_iters in 1 .. {lib.nplda_vbhmm_max_iters()}")
    if (labels_init is None) == (gamma_init is None):
        raise ValueError("give exactly one of labels_init and gamma_init")
    offs = _ragged(offsets, rows, dev)
    if offs.rows != rows:
        raise ValueError(f"the offsets cover {offs.rows} rows, z has {rows}")
    spk = _ragged(spk_offsets, 0, dev) if spk_offsets is not None else None
    if spk is None or spk.P != offs.P:
        raise ValueError("spk_offsets must give one range of speaker slots per problem")
    T, S = offs.host[1:] - offs.host[:-1], spk.host[1:] - spk.host[:-1]
    if ((S == 0) & (T > 0)).any() or (S > lib.nplda_vbhmm_max_speakers()).any():
        raise ValueError(f"every problem with rows needs 1 .. {lib.nplda_vbhmm_max_speakers()} speaker slots")
    n_gamma = int((T * S).sum())
    if labels_init is not None:
        labels_init = torch.as_tensor(labels_init).to(device=dev, dtype=torch.int32).contiguous()
        if labels_init.shape != (rows,):
            raise ValueError("labels_init must hold one label per row of z")
    else:
        gamma_init = torch.as_tensor(gamma_init).to(device=dev, dtype=torch.float64).contiguous().view(-1)
        if gamma_init.numel() != n_gamma:
            raise ValueError(f"gamma_init holds {gamma_init.numel()} posteriors, the offsets ask for {n_gamma}")
    if pi_init is not None:
        pi_init = torch.as_tensor(pi_init).to(device=dev, dtype=torch.float64).contiguous().view(-1)
        if pi_init.numel() != spk.rows:
            raise ValueError(f"pi_init holds {pi_init.numel()} priors, the speaker offsets ask for {spk.rows}")
    gamma = torch.empty(n_gamma, dtype=torch.float64, device=dev)
    pi = torch.empty(spk.rows, dtype=torch.float64, device=dev)
    elbo = torch.empty((offs.P, max_iters), dtype=torch.float64, device=dev)
    n_iters = torch.empty(offs.P, dtype=torch.int32, device=dev)
    labels = torch.empty(rows, dtype=torch.int32, device=dev)
    n_speakers = torch.empty(offs.P, dtype=torch.int32, device=dev)
    if offs.P == 0:
        return gamma, pi, elbo, n_iters, labels, n_speakers
    wsb = lib.nplda_vbhmm_workspace_bytes(offs.hptr, spk.hptr, offs.P, D2)
    if wsb == 0:
        raise _lib.NpldaHipError("vbhmm: the offsets or D2 are outside what the kernel takes")
    ws = torch.empty(wsb // 8, dtype=torch.float64, device=dev)
    if rows == 0:  # no row, no initialiser to read: the entry point still wants exactly one non-null
        labels_init, gamma_init = torch.zeros(1, dtype=torch.int32, device=dev), None
    with _lib.on_device(dev):
        code = lib.nplda_vbhmm_f64(_lib.ptr(z), ldz, offs.hptr, _lib.ptr(offs.dev), spk.hptr, _lib.ptr(spk.dev), offs.P, D2,
                                   _lib.ptr(psi), _lib.ptr(labels_init), _lib.ptr(gamma_init), _lib.ptr(pi_init), Fa, Fb,
                                   loop_prob, epsilon, init_smoothing, max_iters, _lib.ptr(gamma), _lib.ptr(pi), _lib.ptr(elbo),
                                   _lib.ptr(n_iters), _lib.ptr(labels), _lib.ptr(n_speakers), _lib.ptr(ws), wsb,
                                   _lib.current_stream())
    _lib.check(code, "nplda_vbhmm_f64")
    return gamma, pi, elbo, n_iters, labels, n_speakers


DER_MAX_FRAMES = 2 ** 31 - 1  # frames per recording: turn bounds are int32
DER_COUNTS = ("scored", "total", "miss", "fa", "summin", "matched")  # the columns of der()'s counts


def _der_offsets(offsets, dev, name, P=None):
    if not isinstance(offsets, RaggedOffsets):
        offsets = RaggedOffsets(offsets, dev, max_rows=DER_MAX_FRAMES)
    if offsets.dev.device != dev:
        raise ValueError(f"{name} lives on another device")
    if P is not None and offsets.P != P:
        raise ValueError(f"{name} must hold {P} + 1 offsets, got {offsets.P} + 1")
    return offsets


def _der_table(t, rows, cols, name, dev):
    t = torch.as_tensor(t)
    if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise TypeError(f"{name} must hold integers")
    if tuple(t.shape) != ((rows, cols) if cols else (rows,)):
        raise ValueError(f"{name} must be {(rows, cols) if cols else (rows,)}, got {tuple(t.shape)}")
    return t.to(device=dev, dtype=torch.int32).contiguous()


def der_problems(prob_reco, device):
    """The recording of each problem of der(), on the host and on the device -> the pair der() takes as prob_reco.  Make
    one outside a graph capture: building it copies from the host."""
    import numpy as np
    host = np.ascontiguousarray(np.asarray(prob_reco.cpu() if isinstance(prob_reco, torch.Tensor) else prob_reco,
                                           dtype=np.int64).astype(np.int32))
    if host.ndim != 1:
        raise ValueError("prob_reco must name one recording per problem")
    return host, torch.from_numpy(host).to(device)


def der(frame_offsets, ref_offsets, ref_turns, prob_reco, hyp_offsets=None, hyp_turns=None, frame_item=None, item_offsets=None,
        item_labels=None, uem_offsets=None, uem=None, collar=0, skip_overlap=False, n_ref_speakers=None, n_hyp_speakers=None,
        want_matrix=False):
    """nplda_der_i64: the counts of the diarization error rate and the optimal speaker mapping of P problems against Rn
    recordings, in integer frames (include/nplda_hip.h has the definitions).  frame_offsets: Rn + 1 offsets of the
    recordings' frames; ref_offsets: Rn + 1 offsets into ref_turns ((N, 3) begin, end, speaker); uem_offsets / uem ((U, 2)
    begin, end) or neither: every frame of a recording; prob_reco: the recording of each problem, a sequence or what
    der_problems() returns.  The hypotheses come in ONE of two forms: hyp_offsets (P + 1) into hyp_turns ((M, 3)), or
    frame_item (one int32 per frame of every recording: the item that owns it, or -1) with item_offsets (P + 1) into
    item_labels (a speaker or -1 per item of the problem).  Offsets: sequences or RaggedOffsets; tables: integer tensors (any
    other integer array is copied to the device as int32).  collar in frames.  n_ref_speakers / n_hyp_speakers: speakers are
    indices below these (default and most: nplda_der_max_speakers()); a turn or a label outside them counts as absent.
    -> (counts (P, 6) int64 in the order of DER_COUNTS, map_ref (P, 64) int32, C (P, 64, 64) int32 or None), on the device."""
    lib = _lib.load()
    limit = int(lib.nplda_der_max_speakers())
    tables = [t for t in (ref_turns, hyp_turns, frame_item, item_labels, uem) if isinstance(t, torch.Tensor) and t.is_cuda]
    if isinstance(frame_offsets, RaggedOffsets):
        dev = frame_offsets.dev.device
    elif tables:
        dev = tables[0].device
    else:
        dev = torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise ValueError("der runs on a HIP device")
    collar = int(collar)
    n_ref = limit if n_ref_speakers is None else int(n_ref_speakers)
    n_hyp = limit if n_hyp_speakers is None else int(n_hyp_speakers)
    if collar < 0 or not 0 <= n_ref <= limit or not 0 <= n_hyp <= limit:
        raise ValueError(f"collar must not be negative and the speaker limits must lie in 0 .. {limit}")
    fo = _der_offsets(frame_offsets, dev, "frame_offsets")
    ro = _der_offsets(ref_offsets, dev, "ref_offsets", fo.P)
    ref_turns = _der_table(ref_turns, ro.rows, 3, "ref_turns", dev)
    if (uem_offsets is None) != (uem is None):
        raise ValueError("give uem_offsets and uem, or neither")
    uo = None
    if uem_offsets is not None:
        uo = _der_offsets(uem_offsets, dev, "uem_offsets", fo.P)
        uem = _der_table(uem, uo.rows, 2, "uem", dev)
    prepared = isinstance(prob_reco, tuple) and len(prob_reco) == 2 and isinstance(prob_reco[1], torch.Tensor)
    host, pdev = prob_reco if prepared else der_problems(prob_reco, dev)
    P = int(host.shape[0])
    if pdev.device != dev or pdev.dtype != torch.int32 or tuple(pdev.shape) != (P,) or str(host.dtype) != "int32":
        raise ValueError("prob_reco must be what der_problems() returns for this device")
    if P and (int(host.min()) < 0 or int(host.max()) >= fo.P):
        raise ValueError(f"prob_reco must name recordings 0 .. {fo.P - 1}")
    by_turns = hyp_offsets is not None
    if by_turns == (item_offsets is not None):
        raise ValueError("give the hypotheses as hyp_offsets + hyp_turns or as frame_item + item_offsets + item_labels")
    ho = io = None
    if by_turns:
        if frame_item is not None or item_labels is not None or hyp_turns is None:
            raise ValueError("the turn form takes hyp_offsets and hyp_turns alone")
        ho = _der_offsets(hyp_offsets, dev, "hyp_offsets", P)
        hyp_turns = _der_table(hyp_turns, ho.rows, 3, "hyp_turns", dev)
    else:
        if hyp_turns is not None or frame_item is None or item_labels is None:
            raise ValueError("the labelled-items form takes frame_item, item_offsets and item_labels alone")
        io = _der_offsets(item_offsets, dev, "item_offsets", P)
        frame_item = _der_table(frame_item, fo.rows, 0, "frame_item", dev)
        item_labels = _der_table(item_labels, io.rows, 0, "item_labels", dev)
    counts = torch.empty((P, len(DER_COUNTS)), dtype=torch.int64, device=dev)
    map_ref = torch.empty((P, limit), dtype=torch.int32, device=dev)
    C = torch.empty((P, limit, limit), dtype=torch.int32, device=dev) if want_matrix else None
    if P == 0:
        return counts, map_ref, C
    wsb = lib.nplda_der_workspace_bytes(fo.hptr, fo.P)
    if wsb == 0:
        raise _lib.NpldaHipError("der: the frame offsets are outside what the kernel takes")
    ws = torch.empty(wsb // 8, dtype=torch.int64, device=dev)

    def nz(t):  # (an empty tensor has no address worth passing)
        return _lib.ptr(t) if t is not None and t.numel() else None
    with _lib.on_device(dev):
        code = lib.nplda_der_i64(fo.hptr, _lib.ptr(fo.dev), fo.P, ro.hptr, _lib.ptr(ro.dev), nz(ref_turns),
                                 uo.hptr if uo else None, _lib.ptr(uo.dev) if uo else None, nz(uem), collar,
                                 1 if skip_overlap else 0, n_ref, n_hyp, host.ctypes.data, _lib.ptr(pdev), P,
                                 ho.hptr if ho else None, _lib.ptr(ho.dev) if ho else None, nz(hyp_turns), nz(frame_item),
                                 io.hptr if io else None, _lib.ptr(io.dev) if io else None, nz(item_labels),
                                 _lib.ptr(counts), _lib.ptr(map_ref), _lib.ptr(C), _lib.ptr(ws), wsb, _lib.current_stream())
    _lib.check(code, "nplda_der_i64")
    return counts, map_ref, C


def row_stats(S, topn=500, select="lowest"):
    """nplda_row_stats_f32 on an explicit (R, M) float32 score matrix."""
    lib = _lib.load()
    _require_dev_f32(S, "S")
    if S.dim() != 2:
        raise ValueError("S must be (R, M)")
    if S.stride(1) != 1:
        S = S.contiguous()
    R, M = S.shape
    stats = torch.empty((R, 4), dtype=torch.float64, device=S.device)
    if R == 0:
        return stats
    with _lib.on_device(S.device):
        code = lib.nplda_row_stats_f32(_lib.ptr(S), S.stride(0) if R > 1 else M, R, M, int(topn),
                                       1 if select == "lowest" else 0, _lib.ptr(stats), _lib.current_stream())
    _lib.check(code, "nplda_row_stats_f32")
    return stats


def asnorm_apply(raw, ie, it, stats):
    """nplda_asnorm_apply_f64: raw (T,) -> (T, 4) float64 columns znorm, tnorm, snorm, asnorm1."""
    lib = _lib.load()
    dev = stats.device
    if not stats.is_cuda or stats.dtype != torch.float64 or stats.dim() != 2 or stats.shape[1] != 4:
        raise ValueError("stats must be the (R, 4) float64 device tensor returned by cohort_stats/row_stats")
    raw = torch.as_tensor(raw).to(dev).double().contiguous()
    ie, it = _idx(ie, "ie", dev), _idx(it, "it", dev)
    T = raw.shape[0]
    out = torch.empty((T, 4), dtype=torch.float64, device=dev)
    if T == 0:
        return out
    with _lib.on_device(dev):
        code = lib.nplda_asnorm_apply_f64(_lib.ptr(raw), _lib.ptr(ie), _lib.ptr(it), T, _lib.ptr(stats.contiguous()),
                                          stats.shape[0], _lib.ptr(out), _lib.current_stream())
    _lib.check(code, "nplda_asnorm_apply_f64")
    return out


# ---- GaussianBackend ---------------------------------------------------------------------------------

def gb_pack(W1, b1, mu_t, Lam_t, mu_n, Lam_n):
    """gb_pack_params_f32 -> (buffer, D0, D1)."""
    lib = _lib.load()
    ts = []
    for n, t in (("W1", W1), ("b1", b1), ("mu_t", mu_t), ("Lam_t", Lam_t), ("mu_n", mu_n), ("Lam_n", Lam_n)):
        _require_dev_f32(t, n)
        ts.append(t.detach().contiguous())
    D1, D0 = W1.shape
    if mu_t.numel() != 2 * D1 or Lam_t.shape != (2 * D1, 2 * D1) or mu_n.numel() != 2 * D1 or Lam_n.shape != (2 * D1, 2 * D1):
        raise ValueError("paired statistics must have dimension 2 * layer1_LDA_dim")
    if D0 % 4 != 0:
        raise ValueError(f"xvector_dim must be a multiple of 4 (got {D0})")
    nbytes = lib.gb_packed_bytes(D0, D1)
    if nbytes == 0:
        raise _lib.NpldaHipError(f"GaussianBackend {D0}->{D1} is outside the compiled kernel set")
    buf = torch.empty(nbytes // 4, dtype=torch.float32, device=W1.device)
    with _lib.on_device(W1.device):
        code = lib.gb_pack_params_f32(*[_lib.ptr(t) for t in ts], D0, D1, _lib.ptr(buf), nbytes, _lib.current_stream())
    _lib.check(code, "gb_pack_params_f32")
    return buf, D0, D1


def _gb_call(x1, x2, packed, want_s, want_paired, want_rn=False):
    lib = _lib.load()
    buf, D0, D1 = packed
    x1, x2, ld = _pair_rows(x1, x2, D0)
    if x1.shape[0] != x2.shape[0]:
        raise ValueError("x1 and x2 must have the same number of rows")
    B = x1.shape[0]
    s = torch.empty(B, dtype=torch.float32, device=x1.device) if want_s else None
    paired = torch.empty((B, 2 * D1), dtype=torch.float32, device=x1.device) if want_paired else None
    rn = torch.empty(2 * B, dtype=torch.float32, device=x1.device) if want_rn else None
    if B > 0:
        with _lib.on_device(x1.device):
            code = lib.gb_score_pairs_ex_f32(_lib.ptr(x1), _lib.ptr(x2), B, ld, _lib.ptr(buf), D0, D1, _lib.ptr(s),
                                             _lib.ptr(paired), _lib.ptr(rn), _lib.current_stream())
        _lib.check(code, "gb_score_pairs_ex_f32")
    return (s, paired, rn) if want_rn else (s, paired)


def gb_score_pairs(x1, x2, W1, b1, mu_t, Lam_t, mu_n, Lam_n):
    """GaussianBackend.forward: (B, D0) x 2 -> (B,)."""
    return _gb_call(x1, x2, gb_pack(W1, b1, mu_t, Lam_t, mu_n, Lam_n), True, False)[0]


def gb_paired(x1, x2, W1, b1):
    """GaussianBackend.forward_getpaired: (B, D0) x 2 -> (B, 2 D1) = [normalize(LDA x1), normalize(LDA x2)]."""
    D1 = W1.shape[0]
    z = torch.zeros(2 * D1, dtype=torch.float32, device=W1.device)
    Z = torch.zeros((2 * D1, 2 * D1), dtype=torch.float32, device=W1.device)
    return _gb_call(x1, x2, gb_pack(W1, b1, z, Z, z, Z), False, True)[1]


def quadform_pack(W1, b1, M, v, c):
    """gb_pack_quadform_f32: image for S = x^T M x + x^T v + c on x = [normalize(LDA x1); normalize(LDA x2)]."""
    lib = _lib.load()
    for n, t in (("W1", W1), ("b1", b1), ("M", M)):
        _require_dev_f32(t, n)
    D1, D0 = W1.shape
    if M.shape != (2 * D1, 2 * D1) or (v is not None and v.numel() != 2 * D1):
        raise ValueError("M must be (2 D1, 2 D1) and v (2 D1)")
    if D0 % 4 != 0:
        raise ValueError(f"xvector_dim must be a multiple of 4 (got {D0})")
    nbytes = lib.gb_packed_bytes(D0, D1)
    if nbytes == 0:
        raise _lib.NpldaHipError(f"model {D0}->{D1} is outside the compiled kernel set")
    buf = torch.empty(nbytes // 4, dtype=torch.float32, device=W1.device)
    ts = [W1.detach().contiguous(), b1.detach().contiguous(), M.detach().contiguous(),
          None if v is None else v.detach().contiguous()]
    with _lib.on_device(W1.device):
        code = lib.gb_pack_quadform_f32(_lib.ptr(ts[0]), _lib.ptr(ts[1]), _lib.ptr(ts[2]), _lib.ptr(ts[3]), float(c), D0,
                                        D1, _lib.ptr(buf), nbytes, _lib.current_stream())
    _lib.check(code, "gb_pack_quadform_f32")
    return buf, D0, D1


def dplda_pack(W1, b1, wlr, blr, out=None):
    """gb_pack_dplda_f32: the quadratic-form image straight from DPlda's parameters (no host sync, no temporaries).
    out: an image returned earlier, refilled in place (its address may be baked into a captured graph)."""
    lib = _lib.load()
    for n, t in (("W1", W1), ("b1", b1), ("wlr", wlr), ("blr", blr)):
        _require_dev_f32(t, n)
    D1, D0 = W1.shape
    if wlr.numel() != 2 * D1 * D1 + D1 or blr.numel() != 1:
        raise ValueError("logistic_regres must be Linear(2 D1^2 + D1, 1)")
    if D0 % 4 != 0:
        raise ValueError(f"xvector_dim must be a multiple of 4 (got {D0})")
    nbytes = lib.gb_packed_bytes(D0, D1)
    if nbytes == 0:
        raise _lib.NpldaHipError(f"model {D0}->{D1} is outside the compiled kernel set")
    if out is not None and (out[1] != D0 or out[2] != D1 or out[0].numel() * 4 < nbytes or out[0].device != W1.device):
        out = None
    buf = out[0] if out is not None else torch.empty(nbytes // 4, dtype=torch.float32, device=W1.device)
    ts = [t.detach().contiguous() for t in (W1, b1, wlr, blr)]
    with _lib.on_device(W1.device):
        code = lib.gb_pack_dplda_f32(*[_lib.ptr(t) for t in ts], D0, D1, _lib.ptr(buf), nbytes, _lib.current_stream())
    _lib.check(code, "gb_pack_dplda_f32")
    return buf, D0, D1


def quadform_score_pairs(x1, x2, packed):
    """(B, D0) x 2 -> (B,) scores of the packed quadratic form (kernel: MODE_GB of the fused forward)."""
    return _gb_call(x1, x2, packed, True, False)[0]


def quadform_score_rows(y1, y2, packed):
    """gb_score_rows_f32: like quadform_score_pairs with the normalisation step skipped."""
    lib = _lib.load()
    buf, D0, D1 = packed
    y1, y2, ld = _pair_rows(y1, y2, D0, "y1", "y2")
    if y1.shape[0] != y2.shape[0]:
        raise ValueError("y1 and y2 must have the same number of rows")
    B = y1.shape[0]
    s = torch.empty(B, dtype=torch.float32, device=y1.device)
    if B > 0:
        with _lib.on_device(y1.device):
            code = lib.gb_score_rows_f32(_lib.ptr(y1), _lib.ptr(y2), B, ld, _lib.ptr(buf), D0, D1, _lib.ptr(s),
                                         _lib.current_stream())
        _lib.check(code, "gb_score_rows_f32")
    return s


def dplda_quadform(wlr, blr, D1):
    """DPlda's single linear unit over [y1 y2^T + y2 y1^T, y1 y1^T + y2 y2^T, y1 + y2] (utils/models.py:484-490)
    as (M, v, c) of x^T M x + x^T v + c, x = [y1; y2]:  M = [[Ww, Wb], [Wb, Ww]], v = [ws; ws], c = bias."""
    w = wlr.detach().reshape(-1)
    n = D1 * D1
    if w.numel() != 2 * n + D1:
        raise ValueError("logistic_regres.weight must have 2 D1^2 + D1 inputs")
    Wb, Ww, ws = w[:n].reshape(D1, D1), w[n:2 * n].reshape(D1, D1), w[2 * n:]
    M = torch.cat([torch.cat([Ww, Wb], 1), torch.cat([Wb, Ww], 1)], 0).contiguous()
    return M, torch.cat([ws, ws]).contiguous(), (float(blr.detach().reshape(-1)[0]) if blr is not None else 0.0)


def dplda_quadform_image(wlr, D1):
    """nplda_dplda_quadform_f32: ((frag, K, N) of M + M^T, v) for rows_matmul — dplda_quadform + pack_matrix(mode=2)
    in one launch (the input-side backward of DPlda's quadratic form)."""
    lib = _lib.load()
    _require_dev_f32(wlr, "wlr")
    w = wlr.detach().reshape(-1)
    if w.numel() != 2 * D1 * D1 + D1:
        raise ValueError("logistic_regres.weight must have 2 D1^2 + D1 inputs")
    w = w.contiguous()
    K = 2 * D1
    nbytes = lib.nplda_matrix_frag_bytes(K, K)
    if nbytes == 0:
        raise _lib.NpldaHipError(f"a {K} x {K} matrix is outside the resident-matrix GEMM (K <= 512, N % 4 == 0)")
    frag = torch.empty(nbytes // 4, dtype=torch.float32, device=w.device)
    v = torch.empty(K, dtype=torch.float32, device=w.device)
    with _lib.on_device(w.device):
        code = lib.nplda_dplda_quadform_f32(_lib.ptr(w), D1, _lib.ptr(frag), nbytes, _lib.ptr(v), _lib.current_stream())
    _lib.check(code, "nplda_dplda_quadform_f32")
    return (frag, K, K), v


def dplda_grad(paired, g, D1):
    """nplda_dplda_grad_f32: (d logistic_regres.weight (1, 2 D1^2 + D1), d bias (1,)) from the paired rows and g = dL/ds —
    weighted_moments + dplda_fold_grad (same bits) without the fp64 moment matrix in between."""
    lib = _lib.load()
    _require_dev_f32(paired, "paired")
    _require_dev_f32(g, "g")
    B, n = paired.shape
    if n != 2 * D1 or g.numel() != B:
        raise ValueError("paired must be (B, 2 D1) and g (B,)")
    if paired.stride(1) != 1 or paired.stride(0) % 4 != 0 or paired.data_ptr() % 16 != 0:
        paired = paired.contiguous()
    nbytes = lib.nplda_moments_workspace_bytes(B, n)
    if nbytes == 0:
        raise _lib.NpldaHipError(f"paired rows of length {n} are outside the moments kernel")
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=paired.device)
    out = torch.empty(2 * D1 * D1 + D1 + 1, dtype=torch.float32, device=paired.device)
    gg = g.detach().contiguous()
    with _lib.on_device(paired.device):
        code = lib.nplda_dplda_grad_f32(_lib.ptr(paired), B, paired.stride(0), D1, _lib.ptr(gg), _lib.ptr(out),
                                        out.data_ptr() + 4 * (out.numel() - 1), _lib.ptr(ws), nbytes, _lib.current_stream())
    _lib.check(code, "nplda_dplda_grad_f32")
    return out[:-1].view(1, -1), out[-1:]


def dplda_update(paired, g, wlr, blr, m, v, step, lr, beta1, beta2, eps, wd, thetas=(), dtheta=None, image=None, ws=None,
                 grad_out=None, loss=None, loss_sum=None):
    """nplda_dplda_update_f32: the tail of DPlda's recipe step in two launches — weighted moments of the paired rows, then per
    element of [logistic_regres.weight | bias] gradient fold + torch.optim.Adam's update + the new value stored into the
    parameter and into `image` (the (buf, D0, D1) of dplda_pack the next forward scores with).  m / v: flat moments
    [weight | bias | thresholds]; step: device [steps taken, scratch].  loss / loss_sum: optional 0-d float32 / (1,) float64
    device tensors, loss_sum += loss inside the update launch."""
    lib = _lib.load()
    B, n = paired.shape
    if loss_sum is not None and (loss is None or loss.dtype != torch.float32 or loss_sum.dtype != torch.float64):
        raise ValueError("dplda_update: loss must be float32 and loss_sum float64")
    D1 = n // 2
    K = len(thetas)
    if wlr.numel() != 2 * D1 * D1 + D1 or blr.numel() != 1 or m.numel() < wlr.numel() + 1 + K or v.numel() != m.numel():
        raise ValueError("dplda_update: parameter / moment shapes do not belong to a DPlda of this D1")
    if paired.stride(1) != 1 or paired.stride(0) % 4 != 0 or paired.data_ptr() % 16 != 0:
        paired = paired.contiguous()
    nbytes = lib.nplda_moments_workspace_bytes(B, n)
    if nbytes == 0:
        raise _lib.NpldaHipError(f"paired rows of length {n} are outside the moments kernel")
    if ws is None or ws.numel() * 4 < nbytes:
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=paired.device)
    gg = g.detach().contiguous()
    tarr = (ctypes.c_void_p * max(K, 1))(*[t.data_ptr() for t in thetas]) if K else None
    buf, D0 = (image[0], image[1]) if image is not None else (None, 0)
    with _lib.on_device(paired.device):
        code = lib.nplda_dplda_update_f32(_lib.ptr(paired), B, paired.stride(0), D1, _lib.ptr(gg), _lib.ptr(wlr), _lib.ptr(blr),
                                          _lib.ptr(m), _lib.ptr(v), tarr, _lib.ptr(dtheta) if K else None, K, _lib.ptr(step),
                                          float(lr), float(beta1), float(beta2), float(eps), float(wd), _lib.ptr(buf), int(D0),
                                          _lib.ptr(grad_out), _lib.ptr(loss) if loss_sum is not None else None,
                                          _lib.ptr(loss_sum), _lib.ptr(ws), ws.numel() * 4, _lib.current_stream())
    _lib.check(code, "nplda_dplda_update_f32")
    return ws


def dplda_update_loss(paired, s, t, loss_thetas, betas, alpha, kind, wlr, blr, m, v, step, lr, beta1, beta2, eps, wd, thetas=(),
                      image=None, ws=None, grad_out=None, loss_sum=None):
    """nplda_dplda_update_loss_f32: dplda_update with the loss inside its first launch — the moments blocks form dL/ds_i from
    (s, t) themselves, one more block of that launch is the loss kernel (loss, dL/dtheta).  Returns (loss, dtheta, ws), or None
    when the batch is outside the one-block loss (B > 4096 / unaligned): the caller runs loss_fwd_bwd + dplda_update."""
    lib = _lib.load()
    B, n = paired.shape
    D1 = n // 2
    K, LK = len(thetas), len(loss_thetas)
    if wlr.numel() != 2 * D1 * D1 + D1 or blr.numel() != 1 or m.numel() < wlr.numel() + 1 + K or v.numel() != m.numel():
        raise ValueError("dplda_update_loss: parameter / moment shapes do not belong to a DPlda of this D1")
    _require_dev_f32(s, "output")
    _require_dev_f32(t, "target")
    if s.shape != (B,) or t.shape != (B,):
        raise ValueError("output and target must be (B,) tensors")
    if B > 4096 or not s.is_contiguous() or not t.is_contiguous() or s.data_ptr() % 16 or t.data_ptr() % 16:
        return None
    if paired.stride(1) != 1 or paired.stride(0) % 4 != 0 or paired.data_ptr() % 16 != 0:
        paired = paired.contiguous()
    ns = lib.nplda_loss_nsums(LK, kind)
    if ns == 0 or kind == LOSS_HARD_CDET:
        raise _lib.NpldaHipError("dplda_update_loss: unsupported loss kind / number of thresholds")
    nbytes = lib.nplda_moments_workspace_bytes(B, n)
    if nbytes == 0:
        raise _lib.NpldaHipError(f"paired rows of length {n} are outside the moments kernel")
    if ws is None or ws.numel() * 4 < nbytes:
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=paired.device)
    dev = paired.device
    sums = torch.empty(ns, dtype=torch.float64, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    dth = torch.empty(max(LK, 1), dtype=torch.float32, device=dev)
    barr = (ctypes.c_float * max(LK, 1))(*[float(b) for b in betas]) if kind != LOSS_BCE else None
    tarr = (ctypes.c_void_p * max(K, 1))(*[x.data_ptr() for x in thetas]) if K else None
    buf, D0 = (image[0], image[1]) if image is not None else (None, 0)
    with _lib.on_device(dev):
        code = lib.nplda_dplda_update_loss_f32(_lib.ptr(paired), B, paired.stride(0), D1, _lib.ptr(s), _lib.ptr(t), kind,
                                               _theta_array(loss_thetas), barr, LK, float(alpha), _lib.ptr(sums), _lib.ptr(loss),
                                               _lib.ptr(dth), None, _lib.ptr(wlr), _lib.ptr(blr), _lib.ptr(m), _lib.ptr(v), tarr, K,
                                               _lib.ptr(step), float(lr), float(beta1), float(beta2), float(eps), float(wd),
                                               _lib.ptr(buf), int(D0), _lib.ptr(grad_out), _lib.ptr(loss_sum), _lib.ptr(ws),
                                               ws.numel() * 4, _lib.current_stream())
    _lib.check(code, "nplda_dplda_update_loss_f32")
    return loss, dth, ws


def weighted_moments(x, w0, w1=None, out=None):
    """nplda_weighted_moments_f32: x (B, n) fp32, w0/w1 (B,) fp32 -> (cnt (nc,), sum (nc, n), sq (nc, n, n)) doubles,
    nc = 2 if w1 is given else 1.  `out` = a previous result to accumulate into (streamed batches)."""
    lib = _lib.load()
    _require_dev_f32(x, "x")
    _require_dev_f32(w0, "w0")
    if w1 is not None:
        _require_dev_f32(w1, "w1")
    if x.dim() != 2:
        raise ValueError("x must be 2-D")
    B, n = x.shape
    if x.stride(1) != 1 or x.stride(0) % 4 != 0 or x.data_ptr() % 16 != 0:
        x = x.contiguous()
    if n % 4 != 0:
        raise ValueError(f"row length must be a multiple of 4 (got {n})")
    ws = [w0.contiguous()] + ([w1.contiguous()] if w1 is not None else [])
    if any(w.numel() != B for w in ws):
        raise ValueError("weights must have one entry per row")
    nc = len(ws)
    if out is None:
        cnt = torch.empty(nc, dtype=torch.float64, device=x.device)
        sm = torch.empty((nc, n), dtype=torch.float64, device=x.device)
        sq = torch.empty((nc, n, n), dtype=torch.float64, device=x.device)
        acc = 0
    else:
        cnt, sm, sq = out
        if cnt.shape != (nc,) or sm.shape != (nc, n) or sq.shape != (nc, n, n) or sq.dtype != torch.float64:
            raise ValueError("`out` does not match this call")
        acc = 1
    nbytes = lib.nplda_moments_workspace_bytes(B, n)
    if nbytes == 0:
        raise _lib.NpldaHipError(f"row length {n} is outside the compiled kernel set")
    wsb = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    with _lib.on_device(x.device):
        code = lib.nplda_weighted_moments_f32(_lib.ptr(x), B, x.stride(0) if B > 0 else n, n, _lib.ptr(ws[0]),
                                              _lib.ptr(ws[1]) if nc == 2 else None, _lib.ptr(cnt), _lib.ptr(sm),
                                              _lib.ptr(sq), acc, _lib.ptr(wsb), nbytes, _lib.current_stream())
    _lib.check(code, "nplda_weighted_moments_f32")
    return cnt, sm, sq


def class_scatter(table, offs, rows=None, pivot=None, n=None, out=None, validate=True):
    """nplda_class_scatter_f32: with x_k = table[rows[k]][:n] - pivot (rows None: the first offs[-1] rows in order; pivot None:
    0; n None: every column) -> (sum (n,), scatter (n, n), class_sum (S, n)) device doubles, class s = positions
    offs[s] .. offs[s + 1] (offs: S + 1 int64, non-decreasing from 0).  `out` = the (sum, scatter) of a previous call to add
    into (streamed training sets; class_sum is this call's alone).  `validate` checks offs and the row indices (one
    device-to-host sync); the kernel itself only clamps."""
    lib = _lib.load()
    _require_dev_f32(table, "table")
    if table.dim() != 2:
        raise ValueError("table must be 2-D")
    dev = table.device
    n = table.shape[1] if n is None else int(n)
    if n <= 0 or n > table.shape[1]:
        raise ValueError(f"n must be in 1 .. {table.shape[1]}")
    if n % 4 != 0:
        raise ValueError(f"row length must be a multiple of 4 (got {n})")
    if table.stride(1) != 1 or table.stride(0) % 4 != 0 or table.stride(0) < n or table.data_ptr() % 16 != 0:
        table = table.contiguous()
    ldt = table.stride(0) if table.shape[0] > 1 else max(table.shape[1], 4)
    if not isinstance(offs, torch.Tensor) or offs.dtype != torch.int64 or offs.dim() != 1 or offs.numel() < 1:
        raise ValueError("offs must be a 1-D int64 tensor of S + 1 offsets")
    offs = offs.to(dev).contiguous()
    S = offs.numel() - 1
    if rows is not None:
        if rows.dtype != torch.int64 or rows.dim() != 1:
            raise ValueError("rows must be a 1-D int64 tensor")
        rows = rows.to(dev).contiguous()
    if validate:
        o = offs.cpu()
        N = int(o[-1])
        if int(o[0]) != 0 or bool((o[1:] < o[:-1]).any()):
            raise ValueError("offs must start at 0 and not decrease")
        if rows is not None and N > 0 and (rows.numel() != N or int(rows.min()) < 0 or int(rows.max()) >= table.shape[0]):
            raise ValueError("rows must hold offs[-1] indices into the table")
    else:
        N = rows.numel() if rows is not None else int(offs[-1])
    if rows is None and N > table.shape[0]:
        raise ValueError("offs[-1] exceeds the number of table rows")
    if S == 0 and N != 0:
        raise ValueError("rows without a class")
    if pivot is not None:
        _require_dev_f32(pivot, "pivot")
        if pivot.numel() != n:
            raise ValueError(f"pivot must have {n} entries")
        pivot = pivot.contiguous()
        if pivot.data_ptr() % 16 != 0:  # pragma: no cover (torch allocations are >= 256-B aligned; a view may not be)
            pivot = pivot.clone()
    if out is None:
        sm = torch.empty(n, dtype=torch.float64, device=dev)
        sc = torch.empty((n, n), dtype=torch.float64, device=dev)
        acc = 0
    else:
        sm, sc = out
        if sm.shape != (n,) or sc.shape != (n, n) or sm.dtype != torch.float64 or sc.dtype != torch.float64 or \
                not sm.is_contiguous() or not sc.is_contiguous():
            raise ValueError("`out` does not match this call")
        acc = 1
    cs = torch.empty((S, n), dtype=torch.float64, device=dev)
    nbytes = lib.nplda_class_scatter_workspace_bytes(N, S, n)
    if nbytes == 0:
        raise _lib.NpldaHipError(f"row length {n} is outside the compiled kernel set (n % 4 == 0, n <= 512)")
    wsb = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    with _lib.on_device(dev):
        code = lib.nplda_class_scatter_f32(_lib.ptr(table), table.shape[0], ldt, _lib.ptr(rows), N, _lib.ptr(offs), S, n,
                                           _lib.ptr(pivot), _lib.ptr(sm), _lib.ptr(sc), _lib.ptr(cs), acc, _lib.ptr(wsb), nbytes,
                                           _lib.current_stream())
    _lib.check(code, "nplda_class_scatter_f32")
    return sm, sc, cs


def dplda_fold_grad(cnt, sm, sq, D1, reduce=None):
    """(cnt, sum, sq) of paired rows weighted by g = dL/ds -> gradient of DPlda's linear unit (utils/models.py:484-490):
    d wlr = [G12 + G21 | G11 + G22 | s1 + s2] (row-major blocks of G = sum g x x^T), d bias = sum g.
    `reduce` (data parallel): sum-all-reduce of the folded fp64 vector [d wlr | d bias] before it is rounded to fp32,
    so that N ranks give the single-process gradient to fp64 rounding."""
    G = sq[0]
    G11, G12, G21, G22 = G[:D1, :D1], G[:D1, D1:], G[D1:, :D1], G[D1:, D1:]
    dw = torch.cat([(G12 + G21).reshape(-1), (G11 + G22).reshape(-1), sm[0, :D1] + sm[0, D1:], cnt[:1]])
    if reduce is not None:
        dw = reduce(dw)
    return dw[:-1].float().reshape(1, -1), dw[-1:].float()


def _trial_target(target, N, dev):
    """The labels of N trials for the score-evaluation entry points: fp32, flat, on the device of the scores."""
    _require_dev_f32(target, "target")
    t = target.detach().reshape(-1).contiguous()
    if t.numel() != N or t.device != dev:
        raise ValueError("target must hold one label per trial, on the device of the scores")
    return t


def detcost_sweep(scores, target, betas, exact=False, want_eer=False):
    """nplda_detcost_sweep_f32 -> (minc (K,), thr (K,), minc_avg (1,), eer (1,) or None), float32 device tensors."""
    lib = _lib.load()
    _require_dev_f32(scores, "scores")
    s = scores.detach().reshape(-1).contiguous()
    N = s.numel()
    t = _trial_target(target, N, s.device)
    K = len(betas)
    if K < 1:
        raise ValueError("at least one beta")
    nbytes = lib.nplda_detcost_workspace_bytes(N)
    if nbytes == 0:
        raise _lib.NpldaHipError(f"{N} scores are outside the supported range")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=s.device)
    out = torch.empty(2 * K + 2, dtype=torch.float32, device=s.device)
    barr = (ctypes.c_float * K)(*[float(b) for b in betas])
    base = out.data_ptr()
    with _lib.on_device(s.device):
        code = lib.nplda_detcost_sweep_f32(_lib.ptr(s), _lib.ptr(t), N, barr, K, 1 if exact else 0, base, base + 4 * K,
                                           base + 8 * K, (base + 8 * K + 4) if want_eer else None, _lib.ptr(ws), nbytes,
                                           _lib.current_stream())
    _lib.check(code, "nplda_detcost_sweep_f32")
    return out[:K], out[K:2 * K], out[2 * K:2 * K + 1], (out[2 * K + 1:] if want_eer else None)


def _require_dev_float(t, name):
    """_require_dev_f32's twin for the calibration entry points, which take fp32 or fp64 scores."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise _lib.NpldaHipError(f"{name} must live on a HIP device (got {t.device}); there is no CPU path")
    if t.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{name} must be float32 or float64 (got {t.dtype})")
    return "f32" if t.dtype == torch.float32 else "f64"


def _require_dev_f64(t, name, numel=None, device=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise _lib.NpldaHipError(f"{name} must live on a HIP device (got {t.device}); there is no CPU path")
    if t.dtype != torch.float64:
        raise TypeError(f"{name} must be float64 (got {t.dtype})")
    if numel is not None and t.numel() != numel:
        raise ValueError(f"{name} must have {numel} entries (got {t.numel()})")
    if device is not None and t.device != device:
        raise ValueError(f"{name} must live on the device of the scores ({device}, got {t.device})")


def _calib_scores(X, name="scores"):
    """(tensor with unit inner stride, N, K, ldx, type suffix): (N,) is one system; a row-strided view is used as it is."""
    sfx = _require_dev_float(X, name)
    X = X.detach()
    if X.dim() == 1:
        X = X.unsqueeze(1)
    if X.dim() != 2:
        raise ValueError(f"{name} must have shape (N,) or (N, K)")
    N, K = X.shape
    if K < 1 or K > CALIB_MAX_K:
        raise _lib.NpldaHipError(f"{name}: {K} systems are outside the compiled kernel set (1 .. {CALIB_MAX_K})")
    if N > 1 and (X.stride(1) != 1 or X.stride(0) < K):
        X = X.contiguous()
    elif N <= 1:
        X = X.contiguous()
    return X, N, K, (X.stride(0) if N > 1 else K), sfx


def _calib_workspace(lib, N, K, dev):
    nbytes = lib.nplda_calib_workspace_bytes(N, K)
    if nbytes == 0:
        raise _lib.NpldaHipError(f"{N} trials of {K} systems are outside the supported range (N >= 2, K <= {CALIB_MAX_K})")
    return torch.empty(nbytes // 8, dtype=torch.float64, device=dev), nbytes


CALIB_MAX_K = 8
CALIB_REPORT = ("objective", "grad_inf", "iterations", "passes", "converged", "not_finite", "stalled", "n_tgt", "n_non",
                "alpha")


def calib_logreg_pass(scores, target, theta, p_target=0.5, l2=0.0):
    """nplda_calib_logreg_pass_*: scores (N,) or (N, K) fp32 / fp64, target (N,) fp32 0/1, theta (K + 1,) fp64 ->
    (counts (2,) = N_tgt, N_non; J (1,); g (K + 1,); H_upper ((K + 1)(K + 2) / 2,)), device doubles (views of one tensor)."""
    lib = _lib.load()
    X, N, K, ldx, sfx = _calib_scores(scores)
    t = _trial_target(target, N, X.device)
    _require_dev_f64(theta, "theta", K + 1, X.device)
    theta = theta.detach().contiguous()
    ws, nbytes = _calib_workspace(lib, N, K, X.device)
    nh = (K + 1) * (K + 2) // 2
    out = torch.empty(3 + K + 1 + nh, dtype=torch.float64, device=X.device)
    with _lib.on_device(X.device):
        code = getattr(lib, "nplda_calib_logreg_pass_" + sfx)(_lib.ptr(X), N, ldx, K, _lib.ptr(t), _lib.ptr(theta),
                                                              float(p_target), float(l2), _lib.ptr(out), _lib.ptr(ws),
                                                              nbytes, _lib.current_stream())
    _lib.check(code, "nplda_calib_logreg_pass_" + sfx)
    return out[:2], out[2:3], out[3:4 + K], out[4 + K:]


def calib_logreg_fit(scores, target, theta, p_target=0.5, l2=0.0, max_passes=64, tol=1e-10, chunk=8):
    """nplda_calib_logreg_fit_*: damped Newton from `theta` ((K + 1,) device fp64, updated IN PLACE to the last accepted
    value) -> report: (10,) device doubles named by CALIB_REPORT.  chunk=None enqueues the whole budget of max_passes
    (pass, step) launch pairs at once and never synchronises; chunk=c enqueues c pairs at a time and reads the report in
    between (one device-to-host copy), so that a fit that converged does not pay for the no-op launches of the rest."""
    lib = _lib.load()
    X, N, K, ldx, sfx = _calib_scores(scores)
    t = _trial_target(target, N, X.device)
    _require_dev_f64(theta, "theta", K + 1, X.device)
    if not theta.is_contiguous():
        raise ValueError("theta is updated in place: it must be contiguous")
    max_passes = int(max_passes)
    if not 1 <= max_passes <= 256:
        raise ValueError("max_passes must be in 1 .. 256")
    ws, nbytes = _calib_workspace(lib, N, K, X.device)
    report = torch.empty(len(CALIB_REPORT), dtype=torch.float64, device=X.device)
    fn = getattr(lib, "nplda_calib_logreg_fit_" + sfx)
    left, resume = max_passes, 0
    with _lib.on_device(X.device):
        while left > 0:
            n = left if chunk is None else min(int(chunk), left)
            code = fn(_lib.ptr(X), N, ldx, K, _lib.ptr(t), _lib.ptr(theta), float(p_target), float(l2), n, float(tol),
                      resume, _lib.ptr(report), _lib.ptr(ws), nbytes, _lib.current_stream())
            _lib.check(code, "nplda_calib_logreg_fit_" + sfx)
            left -= n
            resume = 1
            if left > 0 and bool(report[4:7].any().item()):  # converged, not finite or stalled
                break
    return report


def calib_gauss_fit(scores, target):
    """nplda_calib_gauss_fit_*: (N,) scores fp32 / fp64, target (N,) fp32 0/1 -> (6,) device doubles: count, mean, population
    standard deviation of the targets, then of the non-targets."""
    lib = _lib.load()
    sfx = _require_dev_float(scores, "scores")
    s = scores.detach().reshape(-1).contiguous()
    N = s.numel()
    t = _trial_target(target, N, s.device)
    ws, nbytes = _calib_workspace(lib, N, 1, s.device)
    out = torch.empty(6, dtype=torch.float64, device=s.device)
    with _lib.on_device(s.device):
        code = getattr(lib, "nplda_calib_gauss_fit_" + sfx)(_lib.ptr(s), _lib.ptr(t), N, _lib.ptr(out), _lib.ptr(ws), nbytes,
                                                            _lib.current_stream())
    _lib.check(code, "nplda_calib_gauss_fit_" + sfx)
    return out


def calib_apply_linear(scores, theta, out_dtype=torch.float64):
    """nplda_calib_apply_linear_*: scores (N,) or (N, K), theta (K + 1,) device fp64 -> (N,) of out_dtype (fp32 / fp64)."""
    lib = _lib.load()
    X, N, K, ldx, sfx = _calib_scores(scores)
    _require_dev_f64(theta, "theta", K + 1, X.device)
    if out_dtype not in (torch.float32, torch.float64):
        raise TypeError("out_dtype must be float32 or float64")
    theta = theta.detach().contiguous()
    out = torch.empty(N, dtype=out_dtype, device=X.device)
    with _lib.on_device(X.device):
        code = getattr(lib, "nplda_calib_apply_linear_" + sfx)(_lib.ptr(X), N, ldx, K, _lib.ptr(theta), _lib.ptr(out),
                                                               int(out_dtype == torch.float64), _lib.current_stream())
    _lib.check(code, "nplda_calib_apply_linear_" + sfx)
    return out


def calib_apply_gauss(scores, mu_tgt, std_tgt, mu_imp, std_imp, out_dtype=torch.float64):
    """nplda_calib_apply_gauss_*: the difference of the two normal log densities at every score (any shape, kept)."""
    lib = _lib.load()
    sfx = _require_dev_float(scores, "scores")
    if out_dtype not in (torch.float32, torch.float64):
        raise TypeError("out_dtype must be float32 or float64")
    s = scores.detach().contiguous()
    out = torch.empty(s.shape, dtype=out_dtype, device=s.device)
    with _lib.on_device(s.device):
        code = getattr(lib, "nplda_calib_apply_gauss_" + sfx)(_lib.ptr(s), s.numel(), float(mu_tgt), float(std_tgt),
                                                              float(mu_imp), float(std_imp), _lib.ptr(out),
                                                              int(out_dtype == torch.float64), _lib.current_stream())
    _lib.check(code, "nplda_calib_apply_gauss_" + sfx)
    return out


def calib_costs(llr, target, thresholds=()):
    """nplda_calib_costs_*: llr (N,) fp32 / fp64, target (N,) fp32 0/1, up to 8 thresholds (floats, +-inf allowed) ->
    (counts (2,) int64 = N_tgt, N_non; miss (nth,) int64; fa (nth,) int64; cllr_sums (2,) fp64 in bits), on the device."""
    lib = _lib.load()
    sfx = _require_dev_float(llr, "llr")
    s = llr.detach().reshape(-1).contiguous()
    N = s.numel()
    t = _trial_target(target, N, s.device)
    nth = len(thresholds)
    if nth > 8:
        raise _lib.NpldaHipError("at most 8 thresholds per call")
    ws, nbytes = _calib_workspace(lib, max(N, 2), 1, s.device)
    counts = torch.empty(2 + 2 * nth, dtype=torch.int64, device=s.device)
    sums = torch.empty(2, dtype=torch.float64, device=s.device)
    tarr = (ctypes.c_double * max(nth, 1))(*[float(v) for v in thresholds])
    with _lib.on_device(s.device):
        code = getattr(lib, "nplda_calib_costs_" + sfx)(_lib.ptr(s), _lib.ptr(t), N, tarr, nth, _lib.ptr(counts),
                                                        _lib.ptr(sums), _lib.ptr(ws), nbytes, _lib.current_stream())
    _lib.check(code, "nplda_calib_costs_" + sfx)
    return counts[:2], counts[2:2 + nth], counts[2 + nth:], sums


PAV_SUMMARY = ("n_tgt", "n_non", "bins", "blocks", "min_cllr", "rocch_eer", "overflow", "reserved")


def pav_chunk():
    """Points one thread scans at level 0 of the hull (nplda_pav_chunk)."""
    return int(_lib.load().nplda_pav_chunk())


def pav_fit(scores, target, laplace=True, cap=None):
    """nplda_pav_fit_*: scores (N,) fp32 / fp64, target (N,) fp32 -> (lo, hi, n, t, llr, summary): the block table of
    the isotonic regression of the labels on the scores (lo, hi, llr fp64; n, t int64; `cap` entries each, of which the
    first min(blocks, cap) are written) and summary (8,) device doubles named by PAV_SUMMARY.  Nothing is read back:
    summary[3] is the true number of blocks and summary[6] tells whether it exceeded cap (default min(N + 2, 65536))."""
    lib = _lib.load()
    sfx = _require_dev_float(scores, "scores")
    s = scores.detach().reshape(-1).contiguous()
    N = s.numel()
    t = _trial_target(target, N, s.device)
    cap = min(N + 2, 1 << 16) if cap is None else int(cap)
    if cap < 1:
        raise ValueError("cap must be at least 1")
    nbytes = lib.nplda_pav_workspace_bytes(N, int(sfx == "f64"))
    if nbytes == 0:
        raise _lib.NpldaHipError(f"{N} trials are outside the supported range (2 <= N < 2^31)")
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=s.device)
    fl = torch.empty(3 * cap + 8, dtype=torch.float64, device=s.device)
    it = torch.empty(2 * cap, dtype=torch.int64, device=s.device)
    lo, hi, llr, summary = fl[:cap], fl[cap:2 * cap], fl[2 * cap:3 * cap], fl[3 * cap:]
    with _lib.on_device(s.device):
        code = getattr(lib, "nplda_pav_fit_" + sfx)(_lib.ptr(s), _lib.ptr(t), N, 1 if laplace else 0, lo.data_ptr(),
                                                    hi.data_ptr(), it.data_ptr(), it.data_ptr() + 8 * cap, llr.data_ptr(),
                                                    cap, summary.data_ptr(), _lib.ptr(ws), nbytes, _lib.current_stream())
    _lib.check(code, "nplda_pav_fit_" + sfx)
    return lo, hi, it[:cap], it[cap:], llr, summary


def pav_apply(scores, lo, hi, llr, out_dtype=torch.float64):
    """nplda_pav_apply_*: scores (any shape, kept) fp32 / fp64 through the block table lo, hi, llr ((nb,) device fp64)."""
    lib = _lib.load()
    sfx = _require_dev_float(scores, "scores")
    if out_dtype not in (torch.float32, torch.float64):
        raise TypeError("out_dtype must be float32 or float64")
    s = scores.detach().contiguous()
    nb = lo.numel()
    for name, x in (("lo", lo), ("hi", hi), ("llr", llr)):
        _require_dev_f64(x, name, nb, s.device)
    if nb < 1:
        raise ValueError("the block table is empty")
    lo, hi, llr = lo.contiguous(), hi.contiguous(), llr.contiguous()
    out = torch.empty(s.shape, dtype=out_dtype, device=s.device)
    with _lib.on_device(s.device):
        code = getattr(lib, "nplda_pav_apply_" + sfx)(_lib.ptr(s), s.numel(), _lib.ptr(lo), _lib.ptr(hi), _lib.ptr(llr), nb,
                                                      _lib.ptr(out), int(out_dtype == torch.float64), _lib.current_stream())
    _lib.check(code, "nplda_pav_apply_" + sfx)
    return out


BOOTSTRAP_MAX_K = 8


def bootstrap_run():
    """Sorted positions one wave walks (nplda_bootstrap_run)."""
    return int(_lib.load().nplda_bootstrap_run())


def bootstrap_tile():
    """Replicates per tile, the point estimate included (nplda_bootstrap_tile)."""
    return int(_lib.load().nplda_bootstrap_tile())


def _group_ids(g, name, N, dev):
    if not isinstance(g, torch.Tensor) or not g.is_cuda or g.dtype != torch.int32:
        raise TypeError(f"{name} must be an int32 tensor on a HIP device")
    g = g.detach().reshape(-1).contiguous()
    if g.numel() != N or g.device != dev:
        raise ValueError(f"{name} must hold one group id per trial, on the device of the scores")
    return g


def bootstrap_metrics(scores, target, g1, G1, g2=None, G2=0, n_boot=1000, seed=0, betas=(1.0,), llr=False):
    """nplda_bootstrap_f32: scores, target (N,) fp32, g1 / g2 (N,) int32 group ids in [0, G1) / [0, G2) (g2 None: one
    side) -> (out (n_boot + 1, ncol) fp64, totals (n_boot + 1, 2) int64, flags (2,) int64), device tensors; nothing is
    read back.  Columns: min cost per beta, EER, then with llr the actual cost per beta and Cllr; row 0 is the point
    estimate.  flags: trials with a group id out of range (excluded), draw counts that saturated."""
    lib = _lib.load()
    _require_dev_f32(scores, "scores")
    s = scores.detach().reshape(-1).contiguous()
    N = s.numel()
    t = _trial_target(target, N, s.device)
    g1 = _group_ids(g1, "g1", N, s.device)
    G1, G2 = int(G1), int(G2)
    if g2 is None:
        if G2 != 0:
            raise ValueError("G2 must be 0 without g2")
    else:
        g2 = _group_ids(g2, "g2", N, s.device)
        if G2 < 1:
            raise ValueError("g2 needs its number of groups G2 >= 1")
    betas = [float(b) for b in betas]
    K, B = len(betas), int(n_boot)
    if K < 1:
        raise ValueError("at least one beta")
    if K > BOOTSTRAP_MAX_K:
        raise _lib.NpldaHipError(f"{K} cost ratios are outside the compiled kernel set (1 .. {BOOTSTRAP_MAX_K})")
    if B < 1:
        raise ValueError("n_boot must be at least 1")
    nbytes = lib.nplda_bootstrap_workspace_bytes(N, G1, G2, B)
    if nbytes == 0:
        raise _lib.NpldaHipError(f"N = {N}, G1 = {G1}, G2 = {G2}, n_boot = {B} are outside the supported range "
                                 "(2 <= N < 2^31, 1 <= G <= 2^20, n_boot <= 2^20)")
    ncol = K + 1 + (K + 1 if llr else 0)
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=s.device)
    out = torch.empty((B + 1, ncol), dtype=torch.float64, device=s.device)
    totals = torch.empty((B + 1, 2), dtype=torch.int64, device=s.device)
    barr = (ctypes.c_double * K)(*betas)
    with _lib.on_device(s.device):
        code = lib.nplda_bootstrap_f32(_lib.ptr(s), _lib.ptr(t), _lib.ptr(g1), _lib.ptr(g2), N, G1, G2, B,
                                       int(seed) & 0xffffffffffffffff, barr, K, 1 if llr else 0, _lib.ptr(out),
                                       _lib.ptr(totals), _lib.ptr(ws), nbytes, _lib.current_stream())
    _lib.check(code, "nplda_bootstrap_f32")
    return out, totals, ws[:2]
