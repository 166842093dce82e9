"""The diarization error rate without a GPU: hand-worked cases on the numpy twin (tests/der_ref.py), the twin's two ways to
the optimal mapping against each other, the confusion identity, the RTTM / UEM readers, the frame -> window rule that the
labelled-items form relies on, the argument checks of the C entry points (status codes come before any launch), the declared
names and the resources of csrc/nplda_der.hip."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import der_ref as dr
from tests.test_topk_cpu import _resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (name, reference turns, hypothesis turns, T, options) -> scored, total, miss, fa, conf, DER; speakers A, B = 0, 1 and
# x, y = 0, 1.  tests/test_der_gpu.py runs the same table through metrics.der and tools/score_rttm.py.
AB = [(0, 10, 0), (10, 20, 1)]
XY = [(0, 12, 0), (12, 20, 1)]
HAND = [
    # A [0, 10), B [10, 20) against x [0, 12), y [12, 20): x takes A (10 frames), y takes B (8); frames 10, 11 are B under x
    ("plain", AB, XY, 20, dict(collar=0), (20, 20, 0, 0, 2, 0.1)),
    # collar 2: the boundaries 0, 10 (twice) and 20 remove [-2, 2), [8, 12) and [18, 22): frames 2 .. 7 and 12 .. 17 stay,
    # six of A under x and six of B under y: nothing is wrong any more
    ("collar", AB, XY, 20, dict(collar=2), (12, 12, 0, 0, 0, 0.0)),
    # A [0, 10), B [5, 15) against x [0, 10), y [10, 15): frames 5 .. 9 have two reference speakers and one hypothesis
    # speaker (5 missed); C = A-x 10, B-x 5, B-y 5, so x -> A, y -> B match 15 = sum of min: no confusion; 5 / 20
    ("overlap", [(0, 10, 0), (5, 15, 1)], [(0, 10, 0), (10, 15, 1)], 15, dict(collar=0), (15, 20, 5, 0, 0, 0.25)),
    # the same without the overlapped frames 5 .. 9: A-x 5, B-y 5, all matched
    ("skip_overlap", [(0, 10, 0), (5, 15, 1)], [(0, 10, 0), (10, 15, 1)], 15, dict(collar=0, skip_overlap=True),
     (10, 10, 0, 0, 0, 0.0)),
    # a hypothesis-only stretch [15, 20): five frames of false alarm against ten of reference speech
    ("hyp_only", [(0, 10, 0)], [(0, 10, 0), (15, 20, 0)], 20, dict(collar=0), (20, 10, 0, 5, 0, 0.5)),
    # two UEM regions [0, 5) and [10, 15) over the first case: A-x 5, B-x 2 (frames 10, 11), B-y 3: matched 8 of 10
    ("uem", AB, XY, 20, dict(collar=0, uem=[(0, 5), (10, 15)]), (10, 10, 0, 0, 2, 0.2)),
]


@pytest.mark.parametrize("case", HAND, ids=lambda c: c[0])
def test_hand_worked_cases(case):
    _, ref, hyp, T, opt, (scored, total, miss, fa, conf, rate) = case
    for method in ("scipy", "brute"):
        c = dr.der_counts(ref, hyp, T, 2, 2, method=method, **opt)
        assert (c.scored, c.total, c.miss, c.fa, c.conf) == (scored, total, miss, fa, conf)
        assert dr.der_value(c) == rate


def test_der_is_nan_without_reference_speech():
    c = dr.der_counts([], [(0, 5, 0)], 10, 0, 1)
    assert (c.scored, c.total, c.miss, c.fa, c.conf) == (10, 0, 0, 5, 0) and np.isnan(dr.der_value(c))


def test_scipy_equals_brute_force_and_the_confusion_identity():
    """300 seeded small problems: both ways to the optimal mapping agree on `matched`, and conf = sum min(|R|, |H|) - matched
    equals the confusion counted frame by frame under either returned mapping."""
    rng = np.random.default_rng(24)
    for k in range(300):
        T = int(rng.integers(1, 80))
        Sr, Sh = int(rng.integers(0, 6)), int(rng.integers(0, 6))
        ref, hyp = dr.random_turns(rng, T, Sr, 8, 30), dr.random_turns(rng, T, Sh, 8, 30)
        opt = dict(collar=int(rng.integers(0, 3)), skip_overlap=bool(k & 1),
                   uem=[(0, T // 3), (T // 2, T)] if k % 5 == 0 else None)
        a = dr.der_counts(ref, hyp, T, Sr, Sh, method="scipy", **opt)
        b = dr.der_counts(ref, hyp, T, Sr, Sh, method="brute", **opt)
        assert a.matched == b.matched and np.array_equal(a.C, b.C)
        scored = dr.scored_mask(ref, T, Sr, opt["uem"], opt["collar"], opt["skip_overlap"])
        for c in (a, b):
            assert len(set(c.mapping.values())) == len(c.mapping)
            assert dr.conf_by_frames(dr.activity(ref, Sr, T), dr.activity(hyp, Sh, T), scored, c.mapping) == c.conf
        assert a.miss + a.summin == a.total and a.fa + a.summin == int(dr.activity(hyp, Sh, T)[:, scored].sum())


# ---- readers -------------------------------------------------------------------------------------------------------------------------

def test_rttm_round_trip(tmp_path):
    from neuralplda_amd import diarize
    turns = np.array([[0, 0, 150, 3], [0, 150, 151, 7], [0, 120, 400, 3], [1, 5, 5, 2], [1, 1234, 99999, 0], [1, 7, 90, 2]], np.int64)
    ids = ["reco-b", "reco-a"]
    path = tmp_path / "x.rttm"
    diarize.write_rttm(str(path), ids, turns)
    text = path.read_text()
    path.write_text("; a comment\nSPKR-INFO reco-b 1 <NA> <NA> <NA> unknown 3 <NA> <NA>\n\n" + text)
    recs, rows, names = diarize.read_rttm(str(path))
    assert recs == ids and rows.dtype == np.int64 and rows.shape == (6, 4)
    want = sorted(turns.tolist(), key=lambda t: (t[0], t[1], t[2]))
    assert rows[:, :3].tolist() == [t[:3] for t in want]
    assert [names[r][lab] for r, _, _, lab in rows.tolist()] == [str(t[3]) for t in want]
    assert names == [["3", "7"], ["2", "0"]]
    back = np.array([[r, b, e, int(names[r][lab])] for r, b, e, lab in rows.tolist()], np.int64)
    diarize.write_rttm(str(tmp_path / "y.rttm"), recs, back)
    assert (tmp_path / "y.rttm").read_text() == text
    # another frame shift: 0.02 s frames written, read as 0.01 s frames
    diarize.write_rttm(str(path), ids, turns[:3], frame_shift=0.02)
    assert diarize.read_rttm(str(path))[1][:, 1:3].tolist() == [[0, 300], [240, 800], [300, 302]]


@pytest.mark.parametrize("line", ["SPEAKER r 1 0.0 1.0 <NA> <NA>", "SPEAKER r 1 zero 1.0 <NA> <NA> a <NA> <NA>",
                                  "SPEAKER r 1 0.0 -1.0 <NA> <NA> a <NA> <NA>", "SPEAKER r 1 -0.5 1.0 <NA> <NA> a <NA> <NA>"])
def test_malformed_rttm_lines_raise_with_file_and_line(tmp_path, line):
    from neuralplda_amd import diarize
    path = tmp_path / "bad.rttm"
    path.write_text("SPEAKER r 1 0.0 1.0 <NA> <NA> a <NA> <NA>\n" + line + "\n")
    with pytest.raises(ValueError, match=re.escape(f"{path}:2:")):
        diarize.read_rttm(str(path))


def test_uem_reader(tmp_path):
    from neuralplda_amd import diarize
    path = tmp_path / "x.uem"
    path.write_text(";; regions\nb 1 10.0 20.5\na 1 0 3.21\nb 1 0.0 5.0\n\n")
    recs, regions = diarize.read_uem(str(path))
    assert recs == ["b", "a"] and [r.tolist() for r in regions] == [[[0, 500], [1000, 2050]], [[0, 321]]]
    assert diarize.read_uem(str(path), 0.02)[1][1].tolist() == [[0, 160]]
    for n, bad in enumerate(["b 1 10.0", "b 1 x 2.0", "b 1 3.0 2.0", "b 1 -1.0 2.0"]):
        path.write_text("a 1 0 1\n" * n + bad + "\n")
        with pytest.raises(ValueError, match=re.escape(f"{path}:{n + 1}:")):
            diarize.read_uem(str(path))


def test_frame_item_reproduces_the_labels_of_turns():
    """frame_labels(windows, arange(W)) names the window that owns each frame, whatever the labels: looking a label vector up
    through it gives the frames that turns(windows, labels) covers with that label."""
    from neuralplda_amd import diarize
    segments = [np.array([[0, 100], [130, 700]]), np.zeros((0, 2), np.int64), np.array([[5, 40], [50, 51], [60, 400]])]
    windows, _ = diarize.uniform_windows(segments, 144, 24)
    W = windows.shape[0]
    assert W > 20
    rng = np.random.default_rng(3)
    items = diarize.frame_labels(windows, np.arange(W))
    for n_spk in (1, 3, W):
        labels = rng.integers(0, n_spk, W)
        T = 720
        want = np.full((3, T), -1, np.int64)
        for r, b, e, lab in diarize.turns(windows, labels).tolist():
            assert (want[r, b:e] == -1).all()
            want[r, b:e] = lab
        got = np.full((3, T), -1, np.int64)
        for r, _, b0, fl in items:
            got[r, b0:b0 + fl.size] = np.where(fl >= 0, labels[np.maximum(fl, 0)], -1)
        assert np.array_equal(got, want)


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------

NAMES = ["nplda_der_max_speakers", "nplda_der_block", "nplda_der_workspace_bytes", "nplda_der_i64"]


def test_declared_names_are_present(hip_lib):
    from neuralplda_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nplda_hip.h")).read()
    for n in NAMES:
        assert n in _lib.SIGNATURES and hasattr(hip_lib, n) and re.search(r"\b%s\(" % n, hdr), n
    assert hip_lib.nplda_abi_version() == 4
    assert hip_lib.nplda_der_max_speakers() == 64
    assert hip_lib.nplda_der_block() % 64 == 0 and 64 <= hip_lib.nplda_der_block() <= 1024


def _i64(*v):
    return (ctypes.c_int64 * len(v))(*v)


def _i32(*v):
    return (ctypes.c_int32 * len(v))(*v)


def test_abi_sizes_and_argument_checks(hip_lib):
    """Every call stops in the validation code (or at P == 0), so nothing is launched and the device pointers are only fake
    aligned addresses."""
    OK, EINVAL, EUNSUP, ENOSPC = 0, -22, -95, -28
    L = hip_lib
    dummy = ctypes.create_string_buffer(4096)
    p16 = (ctypes.addressof(dummy) + 15) // 16 * 16
    big = 1 << 40
    frames, refs = _i64(0, 0, 300, 1000), _i64(0, 0, 4, 9)
    need = L.nplda_der_workspace_bytes(frames, 3)
    assert need >= 12 * 1000 and need % 256 == 0
    assert L.nplda_der_workspace_bytes(_i64(0), 0) > 0 and L.nplda_der_workspace_bytes(_i64(0, 0), 1) % 256 == 0
    assert L.nplda_der_workspace_bytes(_i64(0, 2 ** 31 - 1), 1) >= 12 * (2 ** 31 - 1)
    for offs, n in ((None, 3), (frames, -1), (_i64(1, 5), 1), (_i64(0, 5, 4), 2), (_i64(0, 2 ** 31), 1), (frames, (1 << 24) + 1)):
        assert L.nplda_der_workspace_bytes(offs, n) == 0

    def der(fh=frames, fd=p16, Rn=3, rh=refs, rd=p16, rt=p16, uh=None, ud=None, ut=None, collar=25, skip=0, sr=64, sh=64,
            ph=_i32(1, 2, 2, 0), pd=p16, P=4, hh=_i64(0, 3, 3, 5, 6), hd=p16, ht=p16, fi=None, ih=None, idv=None, il=None,
            counts=p16, maps=p16, C=None, ws=p16, wsb=big):
        return L.nplda_der_i64(fh, fd, Rn, rh, rd, rt, uh, ud, ut, collar, skip, sr, sh, ph, pd, P, hh, hd, ht, fi, ih, idv, il,
                               counts, maps, C, ws, wsb, None)

    items = dict(hh=None, hd=None, ht=None, fi=p16, ih=_i64(0, 2, 2, 7, 9), idv=p16, il=p16)
    assert der(wsb=0) == ENOSPC and der(wsb=need - 1) == ENOSPC                    # every check but the last passed
    assert der(wsb=0, **items) == ENOSPC and der(wsb=0, C=p16, uh=_i64(0, 1, 1, 3), ud=p16, ut=p16) == ENOSPC
    none = dict(fd=None, rd=None, rt=None, pd=None, hd=None, ht=None, counts=None, maps=None, ws=None)
    assert der(P=0, ph=None, hh=_i64(0)) == OK and der(P=0, ph=None, hh=_i64(0), **none) == OK
    for k in none:
        assert der(**{k: None}) == EINVAL, k
    for k in ("fi", "idv", "il"):
        assert der(**{**items, k: None}) == EINVAL, k
    for kw in (dict(collar=-1), dict(sr=-1), dict(sh=-1), dict(P=-1), dict(Rn=-1), dict(fh=None), dict(rh=None), dict(ph=None),
               dict(fh=_i64(1, 1, 300, 1000)), dict(fh=_i64(0, 400, 300, 1000)), dict(rh=_i64(0, 5, 4, 9)), dict(rh=_i64(2, 2, 4, 9)),
               dict(ph=_i32(1, 2, 3, 0)), dict(ph=_i32(1, -1, 2, 0)), dict(hh=_i64(0, 3, 2, 5, 6)), dict(hh=_i64(1, 3, 3, 5, 6)),
               dict(hh=None), dict(ih=_i64(0, 2, 2, 7, 9)),                        # neither form, both forms
               dict(fi=p16), dict(il=p16), dict(idv=p16), {**items, "ht": p16}, {**items, "hd": p16},   # pointers of the other form
               {**items, "ih": _i64(0, 2, 1, 7, 9)}, dict(uh=_i64(0, 1, 1, 3)), dict(ud=p16), dict(uh=_i64(0, 2, 1, 3), ud=p16, ut=p16),
               dict(uh=_i64(0, 1, 1, 3), ud=p16)):
        assert der(**kw) == EINVAL, kw
    for kw in (dict(fd=p16 + 4), dict(rd=p16 + 4), dict(hd=p16 + 4), dict(counts=p16 + 4), dict(rt=p16 + 2), dict(pd=p16 + 2),
               dict(ht=p16 + 2), dict(maps=p16 + 2), dict(C=p16 + 2), dict(ws=p16 + 8), {**items, "fi": p16 + 2},
               {**items, "il": p16 + 2}, {**items, "idv": p16 + 4}, dict(uh=_i64(0, 1, 1, 3), ud=p16 + 4, ut=p16),
               dict(uh=_i64(0, 1, 1, 3), ud=p16, ut=p16 + 2)):
        assert der(**kw) == EINVAL, kw
    for kw in (dict(sr=65), dict(sh=65), dict(fh=_i64(0, 0, 300, 300 + 2 ** 31)), dict(sr=65, wsb=0)):
        assert der(**kw) == EUNSUP, kw
    assert der(sr=65, collar=-1) == EINVAL                                          # an invalid argument wins
    assert der(sr=65, P=0, ph=None, hh=_i64(0)) == EUNSUP and der(sr=0, sh=0, wsb=0) == ENOSPC


# ---- kernel resources --------------------------------------------------------------------------------------------------------------

def test_resources_of_the_der_kernels():
    """design/k24_der.md: three kernels, none with scratch.  The counting kernel keeps the 64 x 64 int32 matrix (16 KB) and a
    chunk of 4096 hypothesis masks (32 KB) in LDS: three workgroups of four waves per CU (more in flight measured slower)."""
    res = _resources("nplda_der.hip")
    assert len(res) == 3, sorted(res)
    for kernel in ("der_init_kernel", "der_paint_kernel", "der_count_kernel"):
        assert sum(kernel in k for k in res) == 1, (kernel, sorted(res))
    for name, v in res.items():
        assert v["ScratchSize"] == 0, (name, v)
        if "der_count" in name:
            assert 48 * 1024 <= v["LDS"] <= 52 * 1024 and v["VGPRs"] + v["AGPRs"] <= 128 and v["Occupancy"] == 3, (name, v)
