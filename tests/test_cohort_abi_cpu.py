"""Status codes and size queries of the AS-norm entry points of csrc/nplda_cohort.hip, pinned before any HIP call is reached.

Every status-code call below stops in the validation code (or at R == 0 / T == 0, which answer OK before any pointer is looked
at), so nothing is launched and the pointers are only fake aligned addresses.  The order in which the checks fire is part of the
C ABI, and so is every byte count the four size queries answer: callers size their workspaces and prepared states with them.
The cohort sizes of the status cases stay at or below 15 000 columns: above about 15 008 the row kernels' dynamic-LDS limit is
raised (a HIP call) between the workspace-size check and the prepared-state check."""
import ctypes

import pytest

OK, EINVAL, EUNSUP, ENOSPC = 0, -22, -95, -28
BIG = 1 << 40  # "enough workspace"
D = (512, 150, 150)        # the recipe model: NB = 10, ldz = 160
D_UNSUP = (512, 500, 150)  # D0 % 4 == 0, no kernel for D1
D_ODD = (510, 150, 150)    # D0 % 4 != 0
D_BOTH = (510, 500, 150)   # both: D0 % 4 is looked at first
MC = 10_000                # an eligible cohort (fused path) at top-500
M_SMALL = 4000             # below the fused path's 4096 columns


@pytest.fixture(scope="module")
def env(hip_lib):
    class Env:
        pass
    e = Env()
    e.lib = hip_lib
    e.buf = ctypes.create_string_buffer(4096)
    e.p = (ctypes.addressof(e.buf) + 255) // 256 * 256
    return e


def _row_bytes(M):
    return (M + 3) // 4 * 4 * 4


def stats_call(env, prepared=False, expect_ok=False, **over):
    p = env.p
    v = dict(z_rows=p, q_rows=p, R=300, z_coh=p, q_coh=p, M=MC, ldz=160, packed=p, dims=D, topn=500, lowest=1, stats=p, ws=p,
             ws_bytes=BIG, state=p, state_bytes=BIG)
    unknown = set(over) - set(v)
    assert not unknown, unknown
    v.update(over)
    args = [v["z_rows"], v["q_rows"], v["R"], v["z_coh"], v["q_coh"], v["M"], v["ldz"], v["packed"], *v["dims"], v["topn"],
            v["lowest"], v["stats"], v["ws"], v["ws_bytes"]]
    if prepared:
        rc = env.lib.nplda_cohort_stats_prepared_f32(*args, v["state"], v["state_bytes"], None)
    else:
        rc = env.lib.nplda_cohort_stats_f32(*args, None)
    assert (rc == OK) == expect_ok, "a call of this test must stop in the validation code"
    return rc


def prepare_call(env, **over):
    p = env.p
    v = dict(z_coh=p, q_coh=p, M=MC, ldz=160, packed=p, dims=D, topn=500, state=p, state_bytes=BIG)
    unknown = set(over) - set(v)
    assert not unknown, unknown
    v.update(over)
    rc = env.lib.nplda_cohort_prepare_f32(v["z_coh"], v["q_coh"], v["M"], v["ldz"], v["packed"], *v["dims"], v["topn"],
                                          v["state"], v["state_bytes"], None)
    assert rc != OK, "a call of this test must stop in the validation code"
    return rc


@pytest.mark.parametrize("prepared", [False, True])
def test_cohort_stats_counts_and_model(env, prepared):
    def call(**over):
        return stats_call(env, prepared, **over)
    # the counts come before the model
    for dims in (D, D_UNSUP, D_ODD):
        assert call(R=-1, dims=dims) == EINVAL
        assert call(M=-1, dims=dims) == EINVAL
        assert call(topn=0, dims=dims) == EINVAL
        assert call(topn=-3, dims=dims) == EINVAL
    assert call(dims=D_ODD) == EINVAL
    assert call(dims=(512, 0, 150)) == EINVAL
    assert call(dims=(512, 150, -1)) == EINVAL
    assert call(dims=D_BOTH) == EINVAL          # D0 % 4 before the unsupported width
    assert call(dims=D_UNSUP) == EUNSUP
    assert call(dims=(512, 150, 500)) == EUNSUP
    # ... and the model before R == 0, which answers OK before any pointer, the cohort size or the workspace is looked at
    assert call(R=0, dims=D_UNSUP) == EUNSUP
    assert call(R=0, dims=D_ODD) == EINVAL
    nothing = dict(z_rows=None, q_rows=None, z_coh=None, q_coh=None, packed=None, stats=None, ws=None, ws_bytes=0)
    assert stats_call(env, prepared, expect_ok=True, R=0, **nothing) == OK
    assert stats_call(env, prepared, expect_ok=True, R=0, M=0, ldz=0, **nothing) == OK
    assert call(M=0) == EINVAL
    assert call(M=0, dims=D_UNSUP) == EUNSUP
    assert call(M=0x7ffffff1) == EINVAL
    assert call(M=0, z_rows=None, ws_bytes=0) == EINVAL


@pytest.mark.parametrize("prepared", [False, True])
def test_cohort_stats_pointers_rows_and_workspace(env, prepared):
    p = env.p

    def call(**over):
        return stats_call(env, prepared, **over)
    for a in ["z_rows", "q_rows", "z_coh", "q_coh", "packed", "stats", "ws"]:
        assert call(**{a: None}) == EINVAL, a
        assert call(ws_bytes=16, **{a: None}) == EINVAL, a   # pointers before the workspace size
    for a in ["z_rows", "z_coh", "packed", "ws"]:
        assert call(**{a: p + 4}) == EINVAL, a
        assert call(ws_bytes=16, **{a: p + 4}) == EINVAL, a
    assert call(ldz=156) == EINVAL   # ldz < 16 NB
    assert call(ldz=162) == EINVAL   # ldz % 4
    assert call(ldz=156, ws_bytes=16) == EINVAL
    assert call(dims=(512, 170, 170), ldz=160) == EINVAL   # NB = 11 rows are 176 wide
    # the control block plus one score row
    for M in (MC, M_SMALL, 15_000, 9_999):
        need = 256 + _row_bytes(M)
        assert call(M=M, ws_bytes=need - 1) == ENOSPC, M
        assert call(M=M, ws_bytes=0) == ENOSPC, M
    assert call(ws_bytes=16, topn=3000) == ENOSPC


def test_cohort_stats_prepared_state(env):
    p, L = env.p, env.lib

    def call(**over):
        return stats_call(env, True, **over)
    # the entry's own check of `state` comes before everything else, R == 0 included
    for state in (None, p + 16, p + 128):
        assert call(state=state) == EINVAL
        assert call(state=state, R=0) == EINVAL
        assert call(state=state, R=-1, dims=D_UNSUP) == EINVAL
        assert call(state=state, dims=D_UNSUP) == EINVAL
        assert call(state=state, ws_bytes=16) == EINVAL
    assert call(dims=D_UNSUP) == EUNSUP
    # a prepared state belongs to the fused path of exactly this shape: the workspace-size check comes first
    assert call(M=M_SMALL, ws_bytes=16) == ENOSPC
    assert call(M=M_SMALL) == EINVAL               # not eligible: too few columns
    assert call(topn=3000) == EINVAL               # not eligible: too large a share of the cohort
    state = L.nplda_cohort_state_bytes(MC, 500, 150, 150)
    fmin = L.nplda_cohort_fused_min_workspace_bytes(MC, 500, 150, 150)
    assert 0 < state < fmin
    assert call(state_bytes=state - 1) == EINVAL
    assert call(state_bytes=0) == EINVAL
    assert call(ws_bytes=fmin - 1) == EINVAL       # a workspace that would select the spilling path
    assert call(ws_bytes=256 + _row_bytes(MC)) == EINVAL
    assert call(ws_bytes=256 + _row_bytes(MC) - 1) == ENOSPC
    assert call(ws_bytes=fmin - 1, state_bytes=state - 1) == EINVAL


def test_cohort_prepare(env):
    p = env.p

    def call(**over):
        return prepare_call(env, **over)
    for dims in (D, D_UNSUP, D_ODD):
        assert call(M=0, dims=dims) == EINVAL
        assert call(M=-1, dims=dims) == EINVAL
        assert call(topn=0, dims=dims) == EINVAL
        assert call(M=0x7ffffff1, dims=dims) == EINVAL
    assert call(dims=D_ODD) == EINVAL
    assert call(dims=(0, 150, 150)) == EINVAL
    assert call(dims=D_BOTH) == EINVAL
    assert call(dims=D_UNSUP) == EUNSUP
    assert call(dims=D_UNSUP, state=None) == EUNSUP   # the model before the pointers
    for a in ["z_coh", "q_coh", "packed", "state"]:
        assert call(**{a: None}) == EINVAL, a
        assert call(M=M_SMALL, **{a: None}) == EINVAL, a        # pointers before eligibility
        assert call(state_bytes=0, **{a: None}) == EINVAL, a
    for off in (16, 128):
        assert call(state=p + off) == EINVAL
    for a in ["z_coh", "packed"]:
        assert call(**{a: p + 4}) == EINVAL, a
    assert call(ldz=156) == EINVAL
    assert call(ldz=162) == EINVAL
    assert call(ldz=156, M=M_SMALL) == EINVAL
    assert call(M=M_SMALL) == EUNSUP
    assert call(M=4095) == EUNSUP
    assert call(topn=3000) == EUNSUP
    assert call(M=M_SMALL, state_bytes=0) == EUNSUP   # eligibility before the state's size
    need = env.lib.nplda_cohort_state_bytes(MC, 500, 150, 150)
    assert need > 0
    assert call(state_bytes=need - 1) == ENOSPC
    assert call(state_bytes=0) == ENOSPC


def test_row_stats_and_asnorm_apply(env):
    p, L = env.p, env.lib

    def rs(S=p, lds=MC, R=4, M=MC, topn=500, lowest=1, stats=p):
        return L.nplda_row_stats_f32(S, lds, R, M, topn, lowest, stats, None)
    assert rs(R=-1) == EINVAL
    assert rs(M=-1) == EINVAL
    assert rs(topn=0) == EINVAL
    assert rs(R=-1, S=None) == EINVAL
    assert rs(R=0) == OK
    assert rs(R=0, S=None, stats=None, M=0, lds=0) == OK
    assert rs(M=0, lds=0) == EINVAL
    assert rs(S=None) == EINVAL
    assert rs(stats=None) == EINVAL
    assert rs(lds=MC - 1) == EINVAL
    assert rs(lds=0) == EINVAL
    assert rs(M=50_000, lds=49_999) == EINVAL   # still before the dynamic-LDS limit is looked at

    def ap(raw=p, ie=p, it=p, T=10, stats=p, R=5, out=p):
        return L.nplda_asnorm_apply_f64(raw, ie, it, T, stats, R, out, None)
    assert ap(T=-1) == EINVAL
    assert ap(R=-1) == EINVAL
    assert ap(T=-1, raw=None) == EINVAL
    assert ap(T=0) == OK
    assert ap(T=0, raw=None, ie=None, it=None, stats=None, out=None) == OK
    assert ap(T=0, R=-1) == EINVAL
    for a in ["raw", "ie", "it", "stats", "out"]:
        assert ap(**{a: None}) == EINVAL, a
    for a in ["stats", "out"]:
        assert ap(**{a: p + 16}) == EINVAL, a   # rows of four doubles: 32-byte aligned
        assert ap(**{a: p + 8}) == EINVAL, a


# ---- sizes -----------------------------------------------------------------------------------------
SIZE_M = (4095, 4096, 10_000, 24_700, 200_000, 1_200_000)
SIZE_TOPN = (1, 100, 500, 3000)
SIZE_DIMS = ((24, 24), (150, 150), (170, 170), (192, 192))
SIZE_R = (1, 129, 22_000, 10 ** 7)
CAP = 4 << 30


def _recorded(M, topn, di):
    """(workspace_bytes_ex per R, fused minimum, state bytes) of one grid point."""
    if topn in FUSED_TOPN[M] and FUSED[M][di] is not None:
        return FUSED[M][di]
    return (SPILL[M], 0, 0)   # not eligible for the fused path: the spilled matrix, nothing to prepare


def test_size_queries(env):
    L = env.lib
    for M in SIZE_M:
        got = tuple(L.nplda_cohort_workspace_bytes(R, M) for R in SIZE_R)
        assert got == DEFAULT_WS[M], M
        for topn in SIZE_TOPN:
            for di, (D1, D2) in enumerate(SIZE_DIMS):
                ex = tuple(L.nplda_cohort_workspace_bytes_ex(R, M, topn, D1, D2) for R in SIZE_R)
                fmin = L.nplda_cohort_fused_min_workspace_bytes(M, topn, D1, D2)
                state = L.nplda_cohort_state_bytes(M, topn, D1, D2)
                assert (ex, fmin, state) == _recorded(M, topn, di), (M, topn, D1, D2)
                # what holds by construction
                assert all(a <= b for a, b in zip(ex, ex[1:])), (M, topn, D1, D2)   # monotone in R ...
                assert ex[-1] <= CAP + 256                                           # ... up to the 4 GiB cap
                assert (fmin == 0) == (state == 0)
                if fmin:
                    assert state < fmin
                    # the minimum is the fused workspace of one 128-row chunk
                    assert fmin == L.nplda_cohort_workspace_bytes_ex(128, M, topn, D1, D2) == ex[0]
                    assert fmin > 256 + _row_bytes(M)
                else:
                    assert ex[0] == 256 + _row_bytes(M)
    # the zeros, spelled out
    assert L.nplda_cohort_workspace_bytes(0, MC) == 0
    assert L.nplda_cohort_workspace_bytes(-1, MC) == 0
    assert L.nplda_cohort_workspace_bytes(300, 0) == 0
    assert L.nplda_cohort_workspace_bytes_ex(0, MC, 500, 150, 150) == 0
    assert L.nplda_cohort_workspace_bytes_ex(300, 0, 500, 150, 150) == 0
    assert L.nplda_cohort_workspace_bytes_ex(300, MC, 500, 500, 150) == 0
    assert L.nplda_cohort_fused_min_workspace_bytes(0, 500, 150, 150) == 0
    assert L.nplda_cohort_fused_min_workspace_bytes(MC, 500, 150, 500) == 0
    assert L.nplda_cohort_fused_min_workspace_bytes(MC, 0, 150, 150) == 0
    assert L.nplda_cohort_state_bytes(0, 500, 150, 150) == 0
    assert L.nplda_cohort_state_bytes(MC, 500, 500, 150) == 0
    # the default query plans the fused path for top-500 at the widest model, with the spilled matrix as a floor
    assert DEFAULT_WS[10_000][0] == FUSED[10_000][3][1]
    assert DEFAULT_WS[10_000][2] == SPILL[10_000][2]


# recorded sizes (bytes), per R of SIZE_R.  SPILL: the score matrix (whole, or 128-row chunks below 4 GiB) + control block.
SPILL = {
    4095: (16640, 2113792, 360448256, 4294967552),
    4096: (16640, 2113792, 360448256, 4294967552),
    10_000: (40256, 5160256, 880000256, 4290560256),
    24_700: (99056, 12745456, 2173600256, 4287129856),
    200_000: (800256, 103200256, 4198400256, 4198400256),
    1_200_000: (4800256, 619200256, 3686400256, 3686400256),
}
# nplda_cohort_workspace_bytes(R, M)
DEFAULT_WS = {
    4095: (16640, 2113792, 360448256, 4294967552),
    4096: (16640, 2113792, 360448256, 4294967552),
    10_000: (21222912, 25600000, 880000256, 4293260800),
    24_700: (46162432, 54832128, 2173600256, 4294313472),
    200_000: (301368832, 318427136, 4198400256, 4293011968),
    1_200_000: (4800256, 619200256, 3686400256, 3686400256),
}
# the top-N of SIZE_TOPN at which a cohort of M takes the fused path (the sizes do not depend on top-N beyond that) ...
FUSED_TOPN = {4095: (), 4096: (1, 100), 10_000: (1, 100, 500), 24_700: (1, 100, 500), 200_000: (1, 100, 500),
              1_200_000: (1, 100, 500)}
# ... and there, per model of SIZE_DIMS: (nplda_cohort_workspace_bytes_ex per R, nplda_cohort_fused_min_workspace_bytes,
# nplda_cohort_state_bytes); None: the cohort's split image would pass 1 GiB, the shape spills
FUSED = {
    4095: (None, None, None, None),
    4096: (((6319104, 10696192, 754801152, 4291488256), 6319104, 893184),
           ((11269120, 15646208, 759751168, 4292061184), 11269120, 5843200),
           ((12437504, 16814592, 760919552, 4293229568), 12437504, 7011584),
           ((12854784, 17231872, 761336832, 4293646848), 12854784, 7428864)),
    10_000: (((8973312, 13350400, 757455360, 4294142464), 8973312, 2035968),
             ((18494464, 22871552, 766976512, 4294909440), 18494464, 11557120),
             ((20805632, 25182720, 769287680, 4292843520), 20805632, 13868288),
             ((21222912, 25600000, 769704960, 4293260800), 21222912, 14285568)),
    24_700: (((15550464, 19927552, 764032512, 4291965440), 15550464, 4849920),
             ((36327424, 40704512, 784809472, 4290856960), 36327424, 25626880),
             ((45745152, 54414848, 1528263168, 4293896192), 45745152, 30752000),
             ((46162432, 54832128, 1528680448, 4294313472), 46162432, 31169280)),
    200_000: (((98376704, 107046400, 1580894720, 4294509568), 98376704, 38506752),
              ((262169600, 279227904, 3179139584, 4287929344), 262169600, 193911040),
              ((300951552, 318009856, 3217921536, 4292594688), 300951552, 232692992),
              ((301368832, 318427136, 3218338816, 4293011968), 301368832, 233110272)),
    1_200_000: (((554765312, 571823616, 3471735296, 4290533888), 554765312, 230506752), None, None, None),
}
