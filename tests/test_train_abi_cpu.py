"""Status codes of the training entry points of csrc/nplda_backward.hip, pinned before any HIP call is reached.

Every call below fails a validation check on purpose, so nothing is launched and the pointers are only fake
16-byte-aligned addresses.  The order in which the checks fire is part of the C ABI (a caller that probes for EUNSUPPORTED to
fall back must not meet EINVAL instead), and so are the sizes the *_bytes / *_floats queries answer."""
import ctypes

import pytest

OK, EINVAL, EUNSUP, ENOSPC = 0, -22, -95, -28
BIG = 1 << 40  # "enough workspace"
M = (512, 150, 150)   # the recipe model: NB = 10
MS = (64, 32, 32)     # a small one: NB = 2


@pytest.fixture(scope="module")
def env(hip_lib):
    class Env:
        pass
    e = Env()
    e.lib = hip_lib
    e.buf = ctypes.create_string_buffer(4096)
    e.p = (ctypes.addressof(e.buf) + 15) // 16 * 16
    return e


def _ptrs(n, p, null_at=None):
    a = (ctypes.c_void_p * n)(*([p] * n))
    if null_at is not None:
        a[null_at] = None
    return a


def _defaults(p):
    """One valid value per argument name; a call made of these alone would launch, so every case overrides something."""
    return dict(x1=p, x2=p, B=64, ldx=512, io_bf16=0, target=p, gcounts=None, params=_ptrs(6, p), dims=M,
                thetas=_ptrs(4, p), betas=(ctypes.c_float * 4)(99.0, 199.0, 9.0, 19.0), K=2, alpha=15.0, kind=0,
                exp_avg=p, exp_avg_sq=p, step=p, packed=p, ws=p, ws_bytes=BIG, loss=p, loss_sum=None, grad_out=None,
                flat=p, dx1=p, dx2=p, lddx=512, table=p, N=1000, rows1=p, rows2=p, cursor=p, stage=p)


_ADAM = (1e-3, 0.9, 0.999, 1e-8, 0.0)
# argument names in C order; "dims" expands to D0, D1, D2 and "adam" to the five hyper-parameters
_ORDER = {
    "nplda_train_step_f32": "x1 x2 B ldx target params dims thetas betas K alpha kind exp_avg exp_avg_sq step adam packed ws "
                            "ws_bytes loss loss_sum grad_out",
    "nplda_train_step_dx_f32": "x1 x2 B ldx io_bf16 target params dims thetas betas K alpha kind exp_avg exp_avg_sq step adam "
                               "packed ws ws_bytes loss loss_sum grad_out dx1 dx2 lddx",
    "nplda_train_step_rows_f32": "table N ldx rows1 rows2 B target params dims thetas betas K alpha kind exp_avg exp_avg_sq "
                                 "step adam packed ws ws_bytes loss loss_sum grad_out",
    "nplda_train_step_records_f32": "table N ldx cursor stage B params dims thetas betas K alpha kind exp_avg exp_avg_sq step "
                                    "adam packed ws ws_bytes loss loss_sum grad_out",
    "nplda_train_step_grad_f32": "x1 x2 B ldx target gcounts params dims thetas betas K alpha kind step packed ws ws_bytes flat",
    "nplda_train_step_grad_rows_f32": "table N ldx rows1 rows2 B target gcounts params dims thetas betas K alpha kind step "
                                      "packed ws ws_bytes flat",
    "nplda_train_step_grad_dx_f32": "x1 x2 B ldx io_bf16 target gcounts params dims thetas betas K alpha kind step packed ws "
                                    "ws_bytes flat dx1 dx2 lddx",
    "nplda_train_step_apply_f32": "flat params dims thetas betas K alpha kind exp_avg exp_avg_sq step adam packed loss loss_sum",
}
STEP = ["nplda_train_step_f32", "nplda_train_step_dx_f32", "nplda_train_step_rows_f32", "nplda_train_step_records_f32"]
GRAD = ["nplda_train_step_grad_f32", "nplda_train_step_grad_rows_f32", "nplda_train_step_grad_dx_f32"]
DIRECT = ["nplda_train_step_f32", "nplda_train_step_dx_f32", "nplda_train_step_grad_f32", "nplda_train_step_grad_dx_f32"]
TABLE = ["nplda_train_step_rows_f32", "nplda_train_step_records_f32", "nplda_train_step_grad_rows_f32"]
DX = ["nplda_train_step_dx_f32", "nplda_train_step_grad_dx_f32"]


def call(env, name, **over):
    v = _defaults(env.p)
    unknown = set(over) - set(v)
    assert not unknown, unknown
    v.update(over)
    args = []
    for a in _ORDER[name].split():
        if a == "dims":
            args += list(v["dims"])
        elif a == "adam":
            args += list(_ADAM)
        else:
            args.append(v[a])
    rc = getattr(env.lib, name)(*args, None)
    assert rc != OK, "a call of this test must stop in the validation code"
    return rc


def _needs(name):
    return set(_ORDER[name].split())


def _ws_need(env, name, B=64, dims=M, io_bf16=0):
    if name in TABLE:
        return env.lib.nplda_train_step_rows_workspace_bytes(B, *dims)
    if name in DX:
        return env.lib.nplda_train_step_dx_workspace_bytes(B, *dims, io_bf16)
    return env.lib.nplda_train_step_workspace_bytes(B, *dims)


def test_entry_point_own_checks(env):
    p = env.p
    for n in DX:
        assert call(env, n, dx1=None) == EINVAL
        assert call(env, n, dx2=None) == EINVAL
        assert call(env, n, dx1=None, dims=(512, 500, 150)) == EINVAL  # the entry's own check comes before the model's
        assert call(env, n, lddx=508) == EINVAL  # lddx < D0
    for n in GRAD:
        assert call(env, n, flat=None) == EINVAL
        assert call(env, n, flat=None, dims=(512, 500, 150)) == EINVAL
    for n in ["nplda_train_step_rows_f32", "nplda_train_step_grad_rows_f32"]:
        assert call(env, n, rows1=None) == EINVAL
        assert call(env, n, rows2=None) == EINVAL
        assert call(env, n, N=0) == EINVAL
        assert call(env, n, N=0, dims=(512, 500, 150)) == EINVAL
    n = "nplda_train_step_records_f32"
    assert call(env, n, cursor=None) == EINVAL
    assert call(env, n, stage=None) == EINVAL
    assert call(env, n, N=0) == EINVAL
    assert call(env, n, stage=p + 8) == EINVAL
    assert call(env, n, B=0) == EINVAL
    assert call(env, n, B=0, dims=(512, 500, 150)) == EINVAL
    assert call(env, n, B=62) == EUNSUP                          # B % 4: the labels sit behind 16 B bytes of indices
    assert call(env, n, B=62, dims=(510, 150, 150)) == EUNSUP    # ... and that check precedes check_model (D0 % 4: EINVAL)
    assert call(env, n, B=64, dims=(510, 150, 150)) == EINVAL


@pytest.mark.parametrize("name", STEP + GRAD)
def test_model_batch_and_loss_checks(env, name):
    need = _needs(name)
    assert call(env, name, dims=(512, 500, 150)) == EUNSUP
    assert call(env, name, dims=(512, 150, 500)) == EUNSUP
    assert call(env, name, dims=(510, 150, 150)) == EINVAL
    assert call(env, name, dims=(512, 0, 150)) == EINVAL
    # rows through a table: staged k16-step by k16-step
    assert call(env, name, dims=(500, 150, 150), ldx=500, lddx=500, ws_bytes=16) == (EUNSUP if name in TABLE else ENOSPC)
    if "io_bf16" in need:
        assert call(env, name, io_bf16=1, dims=(256, 150, 150), B=0) == EUNSUP
        assert call(env, name, io_bf16=1, dims=(500, 150, 150), B=0) == EUNSUP   # D0 % 16 (bf16 rows are staged too)
        assert call(env, name, io_bf16=1, B=0) == EINVAL                          # D0 = 512 passes that check
        assert call(env, name, dims=(256, 150, 150), ldx=256, lddx=200) == EINVAL
    assert call(env, name, B=0) == EINVAL
    assert call(env, name, B=-4) == EINVAL
    assert call(env, name, B=16385 if name != "nplda_train_step_records_f32" else 16388) == EUNSUP
    assert call(env, name, B=16388, kind=7) == EUNSUP      # batch size before the loss spec
    assert call(env, name, kind=2) == EUNSUP
    assert call(env, name, kind=7) == EINVAL
    assert call(env, name, kind=-1) == EINVAL
    assert call(env, name, kind=2, target=None, thetas=None) == EUNSUP   # the loss spec before the pointers
    assert call(env, name, K=0) == EINVAL
    assert call(env, name, K=5) == EINVAL
    assert call(env, name, K=0, kind=1, ws_bytes=16) == ENOSPC   # BCE has one threshold whatever K says
    assert call(env, name, K=5, kind=1, ws_bytes=16) == ENOSPC
    assert call(env, name, betas=None) == EINVAL
    assert call(env, name, betas=None, kind=1, ws_bytes=16) == ENOSPC
    assert call(env, name, thetas=None) == EINVAL
    assert call(env, name, params=None) == EINVAL
    assert call(env, name, K=0, ws_bytes=16) == EINVAL           # ... and before the workspace size


@pytest.mark.parametrize("name", STEP + GRAD)
def test_pointer_row_and_workspace_checks(env, name):
    p = env.p
    need = _needs(name)
    required = ["step", "packed", "ws"] + [a for a in ("target", "exp_avg", "exp_avg_sq", "loss") if a in need]
    for a in required:
        assert call(env, name, **{a: None}) == EINVAL, a
        assert call(env, name, ws_bytes=16, **{a: None}) == EINVAL, a   # pointers before the workspace size
    for a in ["packed", "ws"] + (["target"] if "target" in need else []):
        assert call(env, name, **{a: p + 4}) == EINVAL, a
    rows = ["x1", "x2"] if name in DIRECT else ["table"]
    for a in rows:
        assert call(env, name, **{a: None}) == EINVAL
        assert call(env, name, **{a: p + 4}) == EINVAL
    assert call(env, name, ldx=508) == EINVAL   # ldx < D0
    assert call(env, name, ldx=514) == EINVAL   # ldx % 4
    for i in range(6):
        assert call(env, name, params=_ptrs(6, p, null_at=i)) == EINVAL
        assert call(env, name, params=_ptrs(6, p, null_at=i), ws_bytes=16) == EINVAL
    ws = _ws_need(env, name)
    assert ws > 0
    assert call(env, name, ws_bytes=ws - 1) == ENOSPC
    th = _ptrs(4, p, null_at=1)
    assert call(env, name, ws_bytes=ws - 1, thetas=th) == ENOSPC   # the per-threshold null check comes after the size check
    assert call(env, name, ws_bytes=ws, thetas=th) == EINVAL
    assert call(env, name, ws_bytes=ws, thetas=_ptrs(4, p, null_at=0), kind=1) == EINVAL
    assert call(env, name, ws_bytes=0, thetas=th) == ENOSPC
    if "io_bf16" in need:  # bf16 rows are staged: the larger workspace
        wsb = _ws_need(env, name, io_bf16=1)
        assert wsb > ws
        assert call(env, name, io_bf16=1, ws_bytes=wsb - 1) == ENOSPC
        assert call(env, name, io_bf16=1, ws_bytes=wsb, thetas=th) == EINVAL
    # what the grad-only entries do not take is not asked for: optional outputs may be null everywhere
    assert call(env, name, ws_bytes=ws, thetas=th, gcounts=None, loss_sum=None, grad_out=None) == EINVAL


def test_apply(env):
    p = env.p
    n = "nplda_train_step_apply_f32"
    assert call(env, n, dims=(512, 500, 150)) == EUNSUP
    assert call(env, n, dims=(510, 150, 150)) == EINVAL
    assert call(env, n, kind=2) == EUNSUP
    assert call(env, n, kind=7) == EINVAL
    assert call(env, n, kind=2, dims=(512, 500, 150), flat=None) == EUNSUP
    assert call(env, n, kind=2, flat=None) == EUNSUP
    assert call(env, n, K=0) == EINVAL
    assert call(env, n, K=5) == EINVAL
    assert call(env, n, betas=None) == EINVAL
    assert call(env, n, thetas=None) == EINVAL
    assert call(env, n, params=None) == EINVAL
    for a in ["flat", "exp_avg", "exp_avg_sq", "step", "packed", "loss"]:
        assert call(env, n, **{a: None}) == EINVAL, a
    assert call(env, n, packed=p + 4) == EINVAL
    for i in range(6):
        assert call(env, n, params=_ptrs(6, p, null_at=i)) == EINVAL
    assert call(env, n, thetas=_ptrs(4, p, null_at=1)) == EINVAL
    assert call(env, n, thetas=_ptrs(4, p, null_at=0), kind=1, K=0, betas=None) == EINVAL  # BCE: K and betas are not looked at


def test_backward_entries(env):
    p, L = env.p, env.lib
    D = M

    def bex(x1=p, x2=p, B=4, ldx=512, packed=p, dims=D, g=p, y=p, z=p, rn=p, ldz=160, P_sqrt=p, ws=p, ws_bytes=BIG,
            grad_flat=p, dx1=None, dx2=None, lddx=512):
        rc = L.nplda_backward_ex_f32(x1, x2, B, ldx, packed, *dims, g, y, z, rn, ldz, P_sqrt, ws, ws_bytes, grad_flat, dx1,
                                     dx2, lddx, None)
        assert rc != OK
        return rc
    assert bex(B=-1) == EINVAL
    assert bex(B=-1, dims=(512, 500, 150)) == EINVAL
    assert bex(dims=(512, 500, 150), grad_flat=None) == EUNSUP
    assert bex(grad_flat=None) == EINVAL
    assert bex(grad_flat=None, B=0) == EINVAL
    assert bex(dx1=p) == EINVAL
    assert bex(dx2=p) == EINVAL
    assert bex(dx1=p, B=0) == EINVAL
    for a in ["packed", "g", "rn", "P_sqrt", "ws", "x1", "x2", "y", "z"]:
        assert bex(**{a: None}) == EINVAL, a
    for a in ["packed", "ws", "x1", "x2", "y", "z"]:
        assert bex(**{a: p + 4}) == EINVAL, a
    assert bex(ldx=508) == EINVAL
    assert bex(ldz=156) == EINVAL
    assert bex(ldz=176) == EINVAL   # ldz != 16 NB
    assert bex(ldz=176, ws_bytes=16) == EINVAL
    assert bex(dx1=p, dx2=p, lddx=508) == EINVAL
    assert bex(dx1=p, dx2=p + 4) == EINVAL
    for want_dx in (0, 1):
        need = L.nplda_backward_ex_workspace_bytes(8, *D, want_dx)
        dx = p if want_dx else None
        assert bex(ws_bytes=need - 1, dx1=dx, dx2=dx) == ENOSPC
    assert L.nplda_backward_ex_workspace_bytes(8, *D, 1) > L.nplda_backward_ex_workspace_bytes(8, *D, 0)
    assert L.nplda_backward_f32(p, p, 4, 512, p, *D, p, p, p, p, 160, p, p, L.nplda_backward_workspace_bytes(4, *D) - 1, p,
                                None) == ENOSPC
    assert L.nplda_backward_f32(p, p, 4, 512, p, *D, p, p, p, p, 160, p, p, BIG, None, None) == EINVAL

    def eb(x=p, N=5, ldx=512, packed=p, dims=D, gz=p, ldgz=152, y=p, rn=p, ldz=160, ws=p, ws_bytes=BIG, grad_flat=p, dx=None,
           lddx=512):
        rc = L.nplda_embed_backward_f32(x, N, ldx, packed, *dims, gz, ldgz, y, rn, ldz, ws, ws_bytes, grad_flat, dx, lddx, None)
        assert rc != OK
        return rc
    assert eb(N=-1) == EINVAL
    assert eb(dims=(512, 500, 150), grad_flat=None) == EUNSUP
    assert eb(grad_flat=None) == EINVAL
    assert eb(ldgz=148) == EINVAL   # ldgz < D2
    for a in ["packed", "gz", "rn", "ws", "x", "y"]:
        assert eb(**{a: None}) == EINVAL, a
    for a in ["packed", "ws", "x", "y"]:
        assert eb(**{a: p + 4}) == EINVAL, a
    assert eb(ldz=176) == EINVAL
    assert eb(dx=p, lddx=508) == EINVAL
    assert eb(dx=p + 4) == EINVAL
    assert eb(ws_bytes=L.nplda_backward_ex_workspace_bytes(5, *D, 0) - 1) == ENOSPC
    assert eb(ws_bytes=L.nplda_backward_ex_workspace_bytes(5, *D, 1) - 1, dx=p) == ENOSPC
    assert eb(ws_bytes=16, ldgz=148) == EINVAL

    def lw(x1=p, x2=p, B=4, ldx=512, du=p, ldz=160, D0=512, D1=150, ws=p, ws_bytes=BIG, out=p):
        rc = L.nplda_lda_wgrad_f32(x1, x2, B, ldx, du, ldz, D0, D1, ws, ws_bytes, out, None)
        assert rc != OK
        return rc
    assert lw(B=-1) == EINVAL
    assert lw(D1=500, out=None) == EUNSUP
    assert lw(out=None) == EINVAL
    assert lw(out=None, B=0) == EINVAL
    for a in ["ws", "x1", "x2", "du"]:
        assert lw(**{a: None}) == EINVAL, a
        assert lw(**{a: p + 4}) == EINVAL, a
        assert lw(ws_bytes=16, **{a: None}) == EINVAL, a   # the pointer checks come first
    assert lw(ldx=508) == EINVAL
    assert lw(ldz=156) == EINVAL
    assert lw(ws_bytes=L.nplda_lda_wgrad_workspace_bytes(4, 512, 150) - 1) == ENOSPC
    assert lw(ws_bytes=0) == ENOSPC


def test_size_queries(env):
    L = env.lib
    assert L.nplda_grad_floats(*M) == SIZES["grad_floats"][0]
    assert L.nplda_grad_floats(*MS) == SIZES["grad_floats"][1]
    assert L.nplda_grad_floats(512, 500, 150) == 0
    assert L.nplda_grad_floats(510, 150, 150) == 0
    assert L.nplda_train_step_flat_floats(*M) == SIZES["grad_floats"][0] + SIZES["flat_extra"]
    assert L.nplda_train_step_flat_floats(*MS) == SIZES["grad_floats"][1] + SIZES["flat_extra"]
    assert L.nplda_train_step_flat_floats(512, 500, 150) == 0
    for mi, dims in enumerate((M, MS)):
        for bi, B in enumerate(SIZE_B):
            got = (L.nplda_train_step_workspace_bytes(B, *dims), L.nplda_train_step_rows_workspace_bytes(B, *dims),
                   L.nplda_train_step_dx_workspace_bytes(B, *dims, 0), L.nplda_train_step_dx_workspace_bytes(B, *dims, 1),
                   L.nplda_backward_workspace_bytes(B, *dims), L.nplda_backward_ex_workspace_bytes(B, *dims, 0),
                   L.nplda_backward_ex_workspace_bytes(B, *dims, 1), L.nplda_lda_wgrad_workspace_bytes(B, dims[0], dims[1]))
            assert got == SIZES["ws"][mi][bi], (dims, B)
    # the zeros, spelled out
    for dims in (M, MS):
        assert L.nplda_train_step_workspace_bytes(0, *dims) == 0
        assert L.nplda_train_step_workspace_bytes(16385, *dims) == 0
        assert L.nplda_train_step_rows_workspace_bytes(0, *dims) == 0
        assert L.nplda_train_step_rows_workspace_bytes(16385, *dims) == 0
        assert L.nplda_train_step_dx_workspace_bytes(0, *dims, 0) == 0
    assert L.nplda_train_step_rows_workspace_bytes(64, 500, 150, 150) == 0   # rows form: D0 % 16
    assert L.nplda_train_step_workspace_bytes(64, 500, 150, 150) > 0
    assert L.nplda_train_step_workspace_bytes(64, 512, 500, 150) == 0
    assert L.nplda_backward_workspace_bytes(-1, *M) == 0
    assert L.nplda_backward_ex_workspace_bytes(-1, *M, 0) == 0
    assert L.nplda_lda_wgrad_workspace_bytes(-1, 512, 150) == 0
    assert L.nplda_lda_wgrad_workspace_bytes(4, 512, 500) == 0


# recorded sizes (bytes); per batch size: train_step, _rows, _dx (fp32 rows), _dx (bf16 rows),
# backward, backward_ex, backward_ex with dx, lda_wgrad
SIZE_B = (0, 1, 100, 4096, 16384, 16385)
SIZES = {
    "grad_floats": [99900, 3200],
    "flat_extra": 72,
    "ws": [
        [(0, 0, 0, 0, 432640, 432640, 760320, 330240),
         (441600, 445696, 441600, 445696, 437760, 435200, 762880, 330240),
         (2264576, 2674176, 2264576, 2674176, 2004480, 1003520, 1331200, 1320960),
         (26957824, 43735040, 26957824, 43735040, 16332800, 10329600, 10657280, 3962880),
         (92256256, 159365120, 92256256, 159365120, 49756160, 27473920, 27801600, 3962880),
         (0, 0, 97024256, 164137216, 54520320, 27476480, 27804160, 7595520)],
        [(0, 0, 0, 0, 12800, 12800, 20992, 8704),
         (15616, 16128, 15616, 16128, 13824, 13312, 21504, 8704),
         (122880, 174080, 122880, 174080, 67584, 40448, 48640, 8704),
         (4669440, 6766592, 4669440, 6766592, 2433024, 1216512, 1224704, 139264),
         (18063360, 26451968, 18063360, 26451968, 9117696, 4661248, 4669440, 139264),
         (0, 0, 18066176, 26455296, 9118720, 4661760, 4669952, 139264)],
    ],
}
