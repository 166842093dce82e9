"""What neuralplda_amd.ops hands to the C ABI for the fused train-step family and the two loss calls, argument by argument.

The tests put a recording proxy in place of the loaded library: every nplda_train_step*_f32 entry point, nplda_loss_finish_f32
and nplda_loss_fwd_bwd_f32 store their positional arguments and return 0, the size queries go to the real library, and
any other entry point fails the test — so no kernel of the library is launched here.  Each recorded tuple is compared with
one written out below in the order include/nplda_hip.h declares: tensors as their data_ptr(), strides and sizes as ints,
scalars as float(), the three ctypes arrays (six parameter pointers, K threshold pointers, K betas) by their contents.

The error table names one malformed argument per entry with the exception it raises today, type and text; where a variant
performs no check, the entry asserts that the call reaches the library.  The table runs behind the same proxy, so that a
check that went missing fails the test instead of launching a kernel on the malformed argument.
"""
import ctypes
import re
import types

import pytest
import torch

from neuralplda_amd import _lib, ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
D0, D1, D2, B, N = 32, 24, 16, 8, 20
_RECORDED = re.compile(r"nplda_train_step\w*_f32$|nplda_loss_finish_f32$|nplda_loss_fwd_bwd_f32$")
_QUERIES = re.compile(r"\w+_bytes$|\w+_flat_floats$|nplda_loss_nsums$|nplda_padded_dim$|nplda_strerror$")


def _dev(t):
    return t.to(DEV)


class _Recorder:
    def __init__(self, real):
        self._real = real
        self.calls = []

    def __getattr__(self, name):
        if _RECORDED.match(name):
            def record(*args):
                self.calls.append((name, args))
                return 0
            return record
        if _QUERIES.match(name):
            return getattr(self._real, name)
        raise AssertionError(f"{name} must not be reached by this test")


@pytest.fixture
def rec(hip_lib, monkeypatch):
    r = _Recorder(hip_lib)
    monkeypatch.setattr(_lib, "load", lambda: r)
    return r


class _Fresh:
    """A 16-byte aligned buffer the wrapper allocated itself: none of the caller's tensors."""

    def __init__(self, a):
        self.taken = {v.data_ptr() for v in vars(a).values() if isinstance(v, torch.Tensor)}


def _vp(ts):
    return ("c_void_p", tuple(t.data_ptr() for t in ts))


def _f32(vals):
    return ("c_float", tuple(ctypes.c_float(float(v)).value for v in vals))


def _assert_call(rec, name, expected):
    assert [n for n, _ in rec.calls] == [name]
    got = rec.calls[0][1]
    assert len(got) == len(expected), (len(got), len(expected))
    for i, (g, e) in enumerate(zip(got, expected)):
        if isinstance(g, ctypes.Array):
            g = (g._type_.__name__, tuple(g))
        if isinstance(e, _Fresh):
            assert type(g) is int and g % 16 == 0 and g not in e.taken, f"{name} argument {i}: {g!r} is not a fresh buffer"
        else:
            assert type(g) is type(e) and g == e, f"{name} argument {i}: {g!r} != {e!r}"
    rec.calls.clear()


def _args(precision="fp32"):
    """Small seeded device tensors for every argument of the family."""
    torch.manual_seed(0)
    real = _lib.load()  # (the recorder: these are size queries)
    a = types.SimpleNamespace()
    a.x1, a.x2 = _dev(torch.randn(B, D0)), _dev(torch.randn(B, D0))
    a.dx1, a.dx2 = _dev(torch.zeros(B, D0)), _dev(torch.zeros(B, D0))
    a.table = _dev(torch.randn(N, D0))
    a.rows1, a.rows2 = _dev(torch.randint(0, N, (B,))), _dev(torch.randint(0, N, (B,)))
    a.target = _dev((torch.rand(B) < 0.3).float())
    a.cursor = _dev(torch.zeros(3, dtype=torch.int64))
    a.stage = _dev(torch.zeros(20 * B, dtype=torch.uint8))
    a.params = [_dev(torch.randn(*sh)) for sh in ((D1, D0), (D1,), (D2, D1), (D2,), (D2,), (D2,))]
    a.thetas = [_dev(torch.randn(1)), _dev(torch.randn(1))]
    a.betas, a.alpha, a.kind = [99.0, 199.0], 15, ops.LOSS_SOFTCDET
    npar = sum(p.numel() for p in a.params) + len(a.thetas)
    a.m, a.v = _dev(torch.zeros(npar)), _dev(torch.zeros(npar))
    a.step = _dev(torch.zeros(1))
    a.lr, a.beta1, a.beta2, a.eps, a.wd = 1e-3, 0.9, 0.999, 1e-8, 1e-5
    nbytes = real.nplda_packed_bytes(D0, D1, D2)
    assert nbytes > 0
    a.packed = ops.PackedParams(_dev(torch.zeros(nbytes // 4)), D0, D1, D2, real.nplda_padded_dim(D1, D2), precision)
    a.ws = _dev(torch.zeros(64))
    a.loss = _dev(torch.zeros(()))
    a.loss_sum = _dev(torch.zeros(1, dtype=torch.float64))
    a.grad_out = _dev(torch.zeros(sum(p.numel() for p in a.params)))
    a.flat = _dev(torch.zeros(int(real.nplda_train_step_flat_floats(D0, D1, D2))))
    a.global_counts = _dev(torch.tensor([3.0, 13.0], dtype=torch.float64))
    a.s, a.sums = _dev(torch.randn(B)), _dev(torch.zeros(int(real.nplda_loss_nsums(2, ops.LOSS_SOFTCDET)), dtype=torch.float64))
    return a


def _adam(a):
    return (float(a.lr), float(a.beta1), float(a.beta2), float(a.eps), float(a.wd))


def _dims_consts(a):
    """params, D0, D1, D2, thetas, betas, K, alpha, kind — the run every entry point of the family shares."""
    return (_vp(a.params), D0, D1, D2, _vp(a.thetas), None if a.kind == ops.LOSS_BCE else _f32(a.betas), len(a.thetas),
            float(a.alpha), a.kind)


def _opt(t):
    return None if t is None else t.data_ptr()


# ---- the calls, positionally as train.py makes them ---------------------------------------------------------------

def _train_step(a, **kw):
    return ops.train_step(a.x1, a.x2, a.target, a.params, a.thetas, a.betas, a.alpha, a.kind, a.m, a.v, a.step, a.lr, a.beta1,
                          a.beta2, a.eps, a.wd, a.packed, a.ws, a.loss, **kw)


def _train_step_rows(a, **kw):
    return ops.train_step_rows(a.table, a.rows1, a.rows2, a.target, a.params, a.thetas, a.betas, a.alpha, a.kind, a.m, a.v,
                               a.step, a.lr, a.beta1, a.beta2, a.eps, a.wd, a.packed, a.ws, a.loss, **kw)


def _train_step_records(a, **kw):
    return ops.train_step_records(a.table, a.cursor, a.stage, B, a.params, a.thetas, a.betas, a.alpha, a.kind, a.m, a.v, a.step,
                                  a.lr, a.beta1, a.beta2, a.eps, a.wd, a.packed, a.ws, a.loss, **kw)


def _train_step_dx(a, **kw):
    return ops.train_step_dx(a.x1, a.x2, a.target, a.params, a.thetas, a.betas, a.alpha, a.kind, a.m, a.v, a.step, a.lr, a.beta1,
                             a.beta2, a.eps, a.wd, a.packed, a.ws, a.loss, a.dx1, a.dx2, **kw)


def _train_step_grad(a, **kw):
    return ops.train_step_grad(a.x1, a.x2, a.target, a.params, a.thetas, a.betas, a.alpha, a.kind, a.step, a.packed, a.ws,
                               a.flat, **kw)


def _train_step_grad_rows(a, **kw):
    return ops.train_step_grad_rows(a.table, a.rows1, a.rows2, a.target, a.params, a.thetas, a.betas, a.alpha, a.kind, a.step,
                                    a.packed, a.ws, a.flat, **kw)


def _train_step_grad_dx(a, **kw):
    return ops.train_step_grad_dx(a.x1, a.x2, a.target, a.params, a.thetas, a.betas, a.alpha, a.kind, a.step, a.packed, a.ws,
                                  a.flat, a.dx1, a.dx2, **kw)


def _train_step_apply(a, **kw):
    return ops.train_step_apply(a.flat, a.params, a.thetas, a.betas, a.alpha, a.kind, a.m, a.v, a.step, a.lr, a.beta1, a.beta2,
                                a.eps, a.wd, a.packed, a.loss, **kw)


def _loss_finish(a, **kw):
    return ops.loss_finish(a.s, a.target, a.thetas, a.betas, a.alpha, a.kind, a.sums, **kw)


def _loss_fwd_bwd(a, **kw):
    return ops.loss_fwd_bwd(a.s, a.target, a.thetas, a.betas, a.alpha, a.kind, **kw)


# ---- the expected tuples, in the order of include/nplda_hip.h -----------------------------------------------------

def _exp_train_step(a, x1, x2, ld, target, loss_sum=None, grad_out=None):
    return ((x1, x2, B, ld, target) + _dims_consts(a) + (a.m.data_ptr(), a.v.data_ptr(), a.step.data_ptr()) + _adam(a)
            + (a.packed.buf.data_ptr(), a.ws.data_ptr(), a.ws.numel() * 4, a.loss.data_ptr(), _opt(loss_sum), _opt(grad_out),
               _lib.current_stream()))


def _exp_train_step_rows(a, target, loss_sum=None, grad_out=None):
    return ((a.table.data_ptr(), N, D0, a.rows1.data_ptr(), a.rows2.data_ptr(), B, target) + _dims_consts(a)
            + (a.m.data_ptr(), a.v.data_ptr(), a.step.data_ptr()) + _adam(a)
            + (a.packed.buf.data_ptr(), a.ws.data_ptr(), a.ws.numel() * 4, a.loss.data_ptr(), _opt(loss_sum), _opt(grad_out),
               _lib.current_stream()))


def _exp_train_step_records(a, loss_sum=None, grad_out=None):
    return ((a.table.data_ptr(), N, D0, a.cursor.data_ptr(), a.stage.data_ptr(), B) + _dims_consts(a)
            + (a.m.data_ptr(), a.v.data_ptr(), a.step.data_ptr()) + _adam(a)
            + (a.packed.buf.data_ptr(), a.ws.data_ptr(), a.ws.numel() * 4, a.loss.data_ptr(), _opt(loss_sum), _opt(grad_out),
               _lib.current_stream()))


def _exp_train_step_dx(a, io_bf16, loss_sum=None):
    return ((a.x1.data_ptr(), a.x2.data_ptr(), B, a.x1.stride(0), io_bf16, a.target.data_ptr()) + _dims_consts(a)
            + (a.m.data_ptr(), a.v.data_ptr(), a.step.data_ptr()) + _adam(a)
            + (a.packed.buf.data_ptr(), a.ws.data_ptr(), a.ws.numel() * 4, a.loss.data_ptr(), _opt(loss_sum), None,
               a.dx1.data_ptr(), a.dx2.data_ptr(), a.dx1.stride(0), _lib.current_stream()))


def _exp_train_step_grad(a, x1, x2, ld, target, global_counts=None):
    return ((x1, x2, B, ld, target, _opt(global_counts)) + _dims_consts(a)
            + (a.step.data_ptr(), a.packed.buf.data_ptr(), a.ws.data_ptr(), a.ws.numel() * 4, a.flat.data_ptr(),
               _lib.current_stream()))


def _exp_train_step_grad_rows(a, target, global_counts=None):
    return ((a.table.data_ptr(), N, D0, a.rows1.data_ptr(), a.rows2.data_ptr(), B, target, _opt(global_counts)) + _dims_consts(a)
            + (a.step.data_ptr(), a.packed.buf.data_ptr(), a.ws.data_ptr(), a.ws.numel() * 4, a.flat.data_ptr(),
               _lib.current_stream()))


def _exp_train_step_grad_dx(a, io_bf16, global_counts=None):
    return ((a.x1.data_ptr(), a.x2.data_ptr(), B, a.x1.stride(0), io_bf16, a.target.data_ptr(), _opt(global_counts))
            + _dims_consts(a)
            + (a.step.data_ptr(), a.packed.buf.data_ptr(), a.ws.data_ptr(), a.ws.numel() * 4, a.flat.data_ptr(),
               a.dx1.data_ptr(), a.dx2.data_ptr(), a.dx1.stride(0), _lib.current_stream()))


def _exp_train_step_apply(a, loss_sum=None):
    return ((a.flat.data_ptr(),) + _dims_consts(a) + (a.m.data_ptr(), a.v.data_ptr(), a.step.data_ptr()) + _adam(a)
            + (a.packed.buf.data_ptr(), a.loss.data_ptr(), _opt(loss_sum), _lib.current_stream()))


def _exp_loss(a, sums, loss, g, dth):
    return ((a.s.data_ptr(), a.target.data_ptr(), B) + _dims_consts(a)[4:]
            + (sums.data_ptr(), loss.data_ptr(), _opt(g), _opt(dth), _lib.current_stream()))


def _misaligned_target():
    t = _dev((torch.rand(B + 1) < 0.3).float())[1:]
    assert t.is_contiguous() and t.data_ptr() % 16 == 4
    return t


def _wide(rows=B):
    """(rows, D0) rows of a (rows, D0 + 4) buffer: unit inner stride, 16-byte aligned, row stride D0 + 4."""
    return _dev(torch.randn(rows, D0 + 4))[:, :D0]


# ---- marshalling ----------------------------------------------------------------------------------------------------

def test_train_step(rec):
    a = _args()
    assert _train_step(a) is a.loss
    _assert_call(rec, "nplda_train_step_f32", _exp_train_step(a, a.x1.data_ptr(), a.x2.data_ptr(), D0, a.target.data_ptr()))
    _train_step(a, grad_out=a.grad_out, loss_sum=a.loss_sum)
    _assert_call(rec, "nplda_train_step_f32",
                 _exp_train_step(a, a.x1.data_ptr(), a.x2.data_ptr(), D0, a.target.data_ptr(), a.loss_sum, a.grad_out))
    a.kind = ops.LOSS_BCE  # no betas
    _train_step(a)
    _assert_call(rec, "nplda_train_step_f32", _exp_train_step(a, a.x1.data_ptr(), a.x2.data_ptr(), D0, a.target.data_ptr()))


def test_train_step_row_strides_and_target_alignment(rec):
    a = _args()
    a.x1, a.x2 = _wide(), _wide()  # the same row stride: passed as they are
    _train_step(a)
    _assert_call(rec, "nplda_train_step_f32", _exp_train_step(a, a.x1.data_ptr(), a.x2.data_ptr(), D0 + 4, a.target.data_ptr()))
    a.x2 = _dev(torch.randn(B, D0))  # different row strides: both made contiguous, ld = D0
    _train_step(a)
    _assert_call(rec, "nplda_train_step_f32", _exp_train_step(a, _Fresh(a), a.x2.data_ptr(), D0, a.target.data_ptr()))
    a.x1 = _dev(torch.randn(B, D0))
    a.target = _misaligned_target()  # cloned
    _train_step(a)
    _assert_call(rec, "nplda_train_step_f32", _exp_train_step(a, a.x1.data_ptr(), a.x2.data_ptr(), D0, _Fresh(a)))


def test_train_step_rows(rec):
    a = _args()
    assert _train_step_rows(a) is a.loss
    _assert_call(rec, "nplda_train_step_rows_f32", _exp_train_step_rows(a, a.target.data_ptr()))
    _train_step_rows(a, grad_out=a.grad_out, loss_sum=a.loss_sum)
    _assert_call(rec, "nplda_train_step_rows_f32", _exp_train_step_rows(a, a.target.data_ptr(), a.loss_sum, a.grad_out))
    a.target = _misaligned_target()
    a.kind = ops.LOSS_BCE
    _train_step_rows(a)
    _assert_call(rec, "nplda_train_step_rows_f32", _exp_train_step_rows(a, _Fresh(a)))


def test_train_step_records(rec):
    a = _args()
    assert _train_step_records(a) is a.loss
    _assert_call(rec, "nplda_train_step_records_f32", _exp_train_step_records(a))
    _train_step_records(a, grad_out=a.grad_out, loss_sum=a.loss_sum)
    _assert_call(rec, "nplda_train_step_records_f32", _exp_train_step_records(a, a.loss_sum, a.grad_out))


@pytest.mark.parametrize("dtype,io_bf16", [(torch.float32, 0), (torch.bfloat16, 1)])
def test_train_step_dx(rec, dtype, io_bf16):
    a = _args()
    a.x1, a.x2, a.dx1, a.dx2 = (t.to(dtype) for t in (a.x1, a.x2, a.dx1, a.dx2))
    assert _train_step_dx(a) is a.loss
    _assert_call(rec, "nplda_train_step_dx_f32", _exp_train_step_dx(a, io_bf16))
    _train_step_dx(a, loss_sum=a.loss_sum)
    _assert_call(rec, "nplda_train_step_dx_f32", _exp_train_step_dx(a, io_bf16, a.loss_sum))
    a.x1, a.x2 = (torch.cat([t, t], 1)[:, :D0] for t in (a.x1, a.x2))  # row stride 2 D0, that of dx1 / dx2 stays D0
    assert a.x1.stride(0) == 2 * D0
    _train_step_dx(a)
    _assert_call(rec, "nplda_train_step_dx_f32", _exp_train_step_dx(a, io_bf16))


def test_train_step_grad(rec):
    a = _args()
    assert _train_step_grad(a) is a.flat
    _assert_call(rec, "nplda_train_step_grad_f32", _exp_train_step_grad(a, a.x1.data_ptr(), a.x2.data_ptr(), D0, a.target.data_ptr()))
    _train_step_grad(a, global_counts=a.global_counts)
    _assert_call(rec, "nplda_train_step_grad_f32",
                 _exp_train_step_grad(a, a.x1.data_ptr(), a.x2.data_ptr(), D0, a.target.data_ptr(), a.global_counts))
    a.x1 = _wide()
    a.target = _misaligned_target()
    a.kind = ops.LOSS_BCE
    _train_step_grad(a)
    _assert_call(rec, "nplda_train_step_grad_f32", _exp_train_step_grad(a, _Fresh(a), a.x2.data_ptr(), D0, _Fresh(a)))


def test_train_step_grad_rows(rec):
    a = _args()
    assert _train_step_grad_rows(a) is a.flat
    _assert_call(rec, "nplda_train_step_grad_rows_f32", _exp_train_step_grad_rows(a, a.target.data_ptr()))
    a.target = _misaligned_target()
    _train_step_grad_rows(a, global_counts=a.global_counts)
    _assert_call(rec, "nplda_train_step_grad_rows_f32", _exp_train_step_grad_rows(a, _Fresh(a), a.global_counts))


@pytest.mark.parametrize("dtype,io_bf16", [(torch.float32, 0), (torch.bfloat16, 1)])
def test_train_step_grad_dx(rec, dtype, io_bf16):
    a = _args()
    a.x1, a.x2, a.dx1, a.dx2 = (t.to(dtype) for t in (a.x1, a.x2, a.dx1, a.dx2))
    assert _train_step_grad_dx(a) is a.flat
    _assert_call(rec, "nplda_train_step_grad_dx_f32", _exp_train_step_grad_dx(a, io_bf16))
    _train_step_grad_dx(a, global_counts=a.global_counts)
    _assert_call(rec, "nplda_train_step_grad_dx_f32", _exp_train_step_grad_dx(a, io_bf16, a.global_counts))


def test_train_step_apply(rec):
    a = _args()
    assert _train_step_apply(a) is a.loss
    _assert_call(rec, "nplda_train_step_apply_f32", _exp_train_step_apply(a))
    a.kind = ops.LOSS_BCE
    _train_step_apply(a, loss_sum=a.loss_sum)
    _assert_call(rec, "nplda_train_step_apply_f32", _exp_train_step_apply(a, a.loss_sum))


def test_loss_finish(rec):
    a = _args()
    loss, g, dth = _loss_finish(a)
    assert g.shape == (B,) and dth.shape == (2,) and loss.dim() == 0
    _assert_call(rec, "nplda_loss_finish_f32", _exp_loss(a, a.sums, loss, g, dth))
    loss, g, dth = _loss_finish(a, want_grad=False)
    assert g is None and dth is None
    _assert_call(rec, "nplda_loss_finish_f32", _exp_loss(a, a.sums, loss, None, None))
    a.kind = ops.LOSS_BCE
    loss, g, dth = _loss_finish(a)
    _assert_call(rec, "nplda_loss_finish_f32", _exp_loss(a, a.sums, loss, g, dth))


def test_loss_fwd_bwd(rec):
    a = _args()
    loss, g, dth, sums = _loss_fwd_bwd(a)
    assert sums.dtype == torch.float64 and sums.numel() == a.sums.numel()
    _assert_call(rec, "nplda_loss_fwd_bwd_f32", _exp_loss(a, sums, loss, g, dth))
    a.kind = ops.LOSS_BCE
    loss, g, dth, sums, joint = _loss_fwd_bwd(a, want_joint=True)
    assert g.data_ptr() == joint.data_ptr() and dth.data_ptr() == joint.data_ptr() + 4 * B and dth.shape == (2,)
    _assert_call(rec, "nplda_loss_fwd_bwd_f32", _exp_loss(a, sums, loss, g, dth))


# ---- the error table ----------------------------------------------------------------------------------------------

def _set(name, make):
    def change(a):
        setattr(a, name, make(a))
    return change


def _param(i, make):
    def change(a):
        a.params = list(a.params)
        a.params[i] = make(a.params[i])
    return change


def _theta(make):
    def change(a):
        a.thetas = [a.thetas[0], make(a.thetas[1])]
    return change


def _bf16_rows(a):
    a.x1, a.x2, a.dx1, a.dx2 = (t.bfloat16() for t in (a.x1, a.x2, a.dx1, a.dx2))


def _noncontig(p):
    return _dev(torch.randn(p.shape[1], p.shape[0])).t()


_CPU = "{} must live on a HIP device (got cpu); there is no CPU path"
_F64 = "{} must be float32 (got torch.float64)"
_IMAGE = "{} needs the fp32 parameter image (pack_params(..., precision='fp32'))"
_INPLACE = "{} updates the parameter tensors in place: they must be contiguous"
_ROWS3 = "x1, x2 and target must have the same number of rows"
_ROWS5 = "x1, x2, target, dx1, dx2 must have the same number of rows"
_LEN3 = "rows1, rows2 and target must have the same length"
_INT64 = "rows must be int64 tensors on the table's device"
_CURSOR = "cursor must be a contiguous int64 tensor of 3 elements on the table's device"
_STAGE = "stage must be a contiguous uint8 tensor of 20 B bytes on the table's device"
_COUNTS = "global_counts must be a contiguous device float64 tensor [N_t, N_n]"
_FLAT = "flat must be a contiguous device float32 tensor of train_step_flat_floats(packed) elements"
_DX_DTYPE = "{}: x1, x2, dx1, dx2 must be device tensors, all float32 or all bfloat16"
_DX_ROWS = "{}: (B, D0) rows with unit inner stride, 16-byte aligned"
_DX_STRIDE = "{}: x1 / x2 (and dx1 / dx2) must share their row stride"
_DX_TARGET = "{}: target must be contiguous and 16-byte aligned"
_LOSS_SHAPE = "output and target must be 1-D tensors of the same length"
_HipError = _lib.NpldaHipError

# (call, the malformed argument, exception type or the entry point the call reaches, message)
_PAIR_ERRORS = [  # shared by train_step and train_step_grad
    (_set("x1", lambda a: a.x1.cpu()), _HipError, _CPU.format("x1")),
    (_set("x2", lambda a: a.x2.cpu()), _HipError, _CPU.format("x2")),
    (_set("x1", lambda a: a.x1.double()), TypeError, _F64.format("x1")),
    (_set("x1", lambda a: a.x1[:, :D0 - 4]), ValueError, f"x1 must have shape (B, {D0}), got ({B}, {D0 - 4})"),
    (_set("x2", lambda a: a.x2[:B - 1]), ValueError, _ROWS3),
    (_set("target", lambda a: a.target[:B - 1]), ValueError, _ROWS3),
    (_set("target", lambda a: a.target.cpu()), _HipError, _CPU.format("target")),
    (_set("target", lambda a: a.target.double()), TypeError, _F64.format("target")),
]
_ROWS_ERRORS = [  # shared by train_step_rows and train_step_grad_rows
    (_set("table", lambda a: a.table.cpu()), _HipError, _CPU.format("table")),
    (_set("rows1", lambda a: a.rows1.int()), TypeError, _INT64),
    (_set("rows2", lambda a: a.rows2.cpu()), TypeError, _INT64),
    (_set("rows2", lambda a: a.rows2[:B - 1]), ValueError, _LEN3),
    (_set("target", lambda a: a.target[:B - 1]), ValueError, _LEN3),
    (_set("target", lambda a: a.target.cpu()), _HipError, _CPU.format("target")),
]
_GRAD_ERRORS = [  # shared by the three train_step_grad forms
    (_set("global_counts", lambda a: a.global_counts.float()), ValueError, _COUNTS),
    (_set("global_counts", lambda a: a.global_counts.cpu()), ValueError, _COUNTS),
    (_set("global_counts", lambda a: _dev(torch.zeros(3, dtype=torch.float64))), ValueError, _COUNTS),
    (_set("global_counts", lambda a: _dev(torch.zeros(4, dtype=torch.float64))[::2]), ValueError, _COUNTS),
    (_set("flat", lambda a: a.flat[:-1]), ValueError, _FLAT),
    (_set("flat", lambda a: a.flat.cpu()), ValueError, _FLAT),
    (_set("flat", lambda a: a.flat.double()), ValueError, _FLAT),
    (_set("flat", lambda a: _dev(torch.zeros(2 * a.flat.numel()))[::2]), ValueError, _FLAT),
    (_theta(lambda t: t.double()), TypeError, _F64.format("theta")),
    (_theta(lambda t: t.cpu()), _HipError, _CPU.format("theta")),
]


def _inplace_errors(what):  # shared by the four forms that update the parameters themselves
    return [
        (_param(0, _noncontig), ValueError, _INPLACE.format(what)),
        (_param(3, lambda p: p.cpu()), _HipError, _CPU.format("parameter")),
        (_param(2, lambda p: p.double()), TypeError, _F64.format("parameter")),
        (_theta(lambda t: t.double()), TypeError, _F64.format("parameter")),
        (_theta(lambda t: _dev(torch.zeros(4))[::2]), ValueError, _INPLACE.format(what)),
    ]


def _dx_errors(what):  # shared by the two dx forms
    return [
        (_set("x1", lambda a: a.x1.cpu()), ValueError, _DX_DTYPE.format(what)),
        (_set("dx1", lambda a: a.dx1.bfloat16()), ValueError, _DX_DTYPE.format(what)),
        (_set("x2", lambda a: a.x2.bfloat16()), ValueError, _DX_DTYPE.format(what)),
        (lambda a: [setattr(a, n, getattr(a, n).double()) for n in ("x1", "x2", "dx1", "dx2")], ValueError, _DX_DTYPE.format(what)),
        (_set("dx2", lambda a: a.dx2[:, :D0 - 4]), ValueError, _DX_ROWS.format(what)),
        (_set("x2", lambda a: _dev(torch.randn(B, D0 + 2))[:, :D0]), ValueError, _DX_ROWS.format(what)),
        (_set("x1", lambda a: _dev(torch.randn(B, D0 + 4))[:, 1:D0 + 1]), ValueError, _DX_ROWS.format(what)),
        (_set("x1", lambda a: _dev(torch.randn(D0, B)).t()), ValueError, _DX_ROWS.format(what)),
        (_set("x2", lambda a: a.x2[:B - 1]), ValueError, _ROWS5),
        (_set("dx2", lambda a: a.dx2[:B - 1]), ValueError, _ROWS5),
        (_set("target", lambda a: a.target[:B - 1]), ValueError, _ROWS5),
        (_set("x2", lambda a: _wide()), ValueError, _DX_STRIDE.format(what)),
        (_set("dx1", lambda a: _wide()), ValueError, _DX_STRIDE.format(what)),
        (_set("target", lambda a: a.target.cpu()), _HipError, _CPU.format("target")),
        (_set("target", lambda a: a.target.double()), TypeError, _F64.format("target")),
        (_set("target", lambda a: _misaligned_target()), ValueError, _DX_TARGET.format(what)),
        (_set("target", lambda a: _dev(torch.zeros(2 * B))[::2]), ValueError, _DX_TARGET.format(what)),
    ]


def _table():
    rows = []

    def add(call, entries):
        rows.extend((call,) + e for e in entries)

    add(_train_step, _PAIR_ERRORS + _inplace_errors("train_step"))
    add(_train_step_grad, _PAIR_ERRORS + _GRAD_ERRORS)
    add(_train_step_rows, _ROWS_ERRORS + _inplace_errors("train_step"))
    add(_train_step_grad_rows, _ROWS_ERRORS + _GRAD_ERRORS)
    add(_train_step_records, [
        (_set("table", lambda a: a.table.cpu()), _HipError, _CPU.format("table")),
        (_set("cursor", lambda a: _dev(torch.zeros(4, dtype=torch.int64))), TypeError, _CURSOR),
        (_set("cursor", lambda a: a.cursor.int()), TypeError, _CURSOR),
        (_set("cursor", lambda a: a.cursor.cpu()), TypeError, _CURSOR),
        (_set("cursor", lambda a: _dev(torch.zeros(6, dtype=torch.int64))[::2]), TypeError, _CURSOR),
        (_set("stage", lambda a: a.stage[:-1]), TypeError, _STAGE),
        (_set("stage", lambda a: _dev(torch.zeros(5 * B))), TypeError, _STAGE),
        (_set("stage", lambda a: a.stage.cpu()), TypeError, _STAGE),
    ] + _inplace_errors("train_step"))
    add(_train_step_dx, _dx_errors("train_step_dx") + _inplace_errors("train_step_dx"))
    add(_train_step_grad_dx, _dx_errors("train_step_grad_dx") + _GRAD_ERRORS)
    # the gradient forms leave the parameter tensors unchecked; train_step_apply checks the image's precision and the
    # thresholds' dtype and device (while it collects their pointers), nothing else
    for call, name in ((_train_step_grad, "nplda_train_step_grad_f32"), (_train_step_grad_rows, "nplda_train_step_grad_rows_f32"),
                       (_train_step_grad_dx, "nplda_train_step_grad_dx_f32"), (_train_step_apply, "nplda_train_step_apply_f32")):
        add(call, [(_param(0, _noncontig), name, None), (_param(3, lambda p: p.cpu()), name, None),
                   (_param(2, lambda p: p.double()), name, None)])
    add(_train_step_apply, [
        (_set("flat", lambda a: a.flat[:-1]), "nplda_train_step_apply_f32", None),
        (_set("flat", lambda a: a.flat.cpu()), "nplda_train_step_apply_f32", None),
        (_set("flat", lambda a: a.flat.double()), "nplda_train_step_apply_f32", None),
        (_theta(lambda t: t.double()), TypeError, _F64.format("theta")),
        (_theta(lambda t: t.cpu()), _HipError, _CPU.format("theta")),
    ])
    for call in (_train_step, _train_step_rows, _train_step_records, _train_step_dx, _train_step_grad, _train_step_grad_rows,
                 _train_step_grad_dx, _train_step_apply):
        add(call, [(_set("packed", lambda a: _args("bf16x3").packed), ValueError, _IMAGE.format(call.__name__[1:]))])
    add(_loss_finish, [
        (_set("s", lambda a: a.s[:B - 1]), "nplda_loss_finish_f32", None),
        (_set("target", lambda a: a.target.double()), "nplda_loss_finish_f32", None),
        (_theta(lambda t: t.double()), TypeError, _F64.format("theta")),
    ])
    add(_loss_fwd_bwd, [
        (_set("s", lambda a: a.s.cpu()), _HipError, _CPU.format("output")),
        (_set("target", lambda a: a.target.cpu()), _HipError, _CPU.format("target")),
        (_set("s", lambda a: a.s.double()), TypeError, _F64.format("output")),
        (_set("target", lambda a: a.target[:B - 1]), ValueError, _LOSS_SHAPE),
        (_set("s", lambda a: a.s.view(2, B // 2)), ValueError, _LOSS_SHAPE),
        (_set("kind", lambda a: ops.LOSS_HARD_CDET), _HipError, "loss_fwd_bwd: unsupported loss kind / number of thresholds"),
        (_theta(lambda t: t.double()), TypeError, _F64.format("theta")),
    ])
    return rows


_TABLE = _table()


@pytest.mark.parametrize("entry", range(len(_TABLE)), ids=[f"{i}-{r[0].__name__[1:]}" for i, r in enumerate(_TABLE)])
def test_error_table(rec, entry):
    call, change, outcome, message = _TABLE[entry]
    a = _args()
    if call in (_train_step_grad, _train_step_grad_rows, _train_step_grad_dx):
        call = _with_counts(call)
    change(a)
    if isinstance(outcome, str):  # no check today: the call reaches the library
        call(a)
        assert [n for n, _ in rec.calls] == [outcome]
        return
    with pytest.raises(outcome) as e:
        call(a)
    assert type(e.value) is outcome and str(e.value) == message
    assert rec.calls == []


def _with_counts(call):
    return lambda a: call(a, global_counts=a.global_counts)


def test_first_failing_check_wins(rec):
    """Inputs that fail several checks: the check that comes first in the wrapper raises."""
    a = _args()
    a.x1, a.target, a.params = a.x1.cpu(), a.target[:B - 1], [_noncontig(a.params[0])] + a.params[1:]
    with pytest.raises(_HipError, match="x1 must live on a HIP device"):
        _train_step(a)
    a = _args()
    a.target, a.params = a.target.cpu()[:B - 1], [_noncontig(a.params[0])] + a.params[1:]
    with pytest.raises(ValueError, match=_ROWS3):
        _train_step(a)
    a = _args()
    a.target, a.params = a.target.cpu(), [_noncontig(a.params[0])] + a.params[1:]
    with pytest.raises(_HipError, match="target must live on a HIP device"):
        _train_step(a)
    a = _args()
    a.rows1, a.target, a.flat = a.rows1.int(), a.target.cpu(), a.flat[:-1]
    with pytest.raises(TypeError, match="rows must be int64"):
        _train_step_grad_rows(a)
    a = _args()
    a.global_counts, a.flat, a.thetas = a.global_counts.float(), a.flat[:-1], [t.double() for t in a.thetas]
    with pytest.raises(ValueError, match="global_counts must be"):
        _train_step_grad(a, global_counts=a.global_counts)
    with pytest.raises(ValueError, match="flat must be"):
        _train_step_grad(a)
    a = _args()
    _bf16_rows(a)
    a.x2, a.target = a.x2[:B - 1], _misaligned_target()
    with pytest.raises(ValueError, match=_ROWS5):
        _train_step_dx(a)
    a = _args()
    a.cursor, a.stage = a.cursor.int(), a.stage[:-1]
    with pytest.raises(TypeError, match="cursor must be"):
        _train_step_records(a)
    assert rec.calls == []
