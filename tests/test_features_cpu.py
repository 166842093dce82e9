"""The host side of the feature front end (neuralplda_amd/kaldi_format.py feature readers, features.VadOptions) and the
build-time facts of its kernels (csrc/nplda_feat.hip): no GPU needed."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from neuralplda_amd import kaldi_format as kf
from tests import feat_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("nplda_feat_decode_f32", "nplda_feat_vad_energy_f32", "nplda_feat_workspace_bytes",
                    "nplda_feat_cmn_select_f32")
NEW_KERNELS = ("feat_decode_kernel", "feat_vad_kernel", "feat_count_kernel", "feat_scan_kernel", "feat_cmn_select_kernel")


def _ulp4(min_value, rng):
    big = np.float32(max(abs(np.float32(min_value)), abs(np.float32(min_value) + np.float32(rng))))
    return 4.0 * float(np.spacing(big))


# ---- 1. hand-written byte strings (share no code with tests/feat_ref.py) ------------------------------------------------

def test_cm3_bytes_by_hand():
    # min_value -1, range 2, 2 x 3, row-major bytes: b -> -1 + 2 b / 255
    obj = b"\0BCM3 " + struct.pack("<ffii", -1.0, 2.0, 2, 3) + bytes([0, 255, 51, 102, 153, 204])
    want = np.array([[-1.0, 1.0, -0.6], [-0.2, 0.2, 0.6]])
    got = kf.read_matrix(obj)
    assert got.shape == (2, 3) and got.dtype == np.float64
    assert np.abs(got - want).max() <= _ulp4(-1.0, 2.0)


def test_cm2_bytes_by_hand():
    # min_value 10, range 5, 3 x 2, row-major uint16: v -> 10 + 5 v / 65535, and 65535 / 5 = 13107
    vals = [0, 65535, 13107, 26214, 39321, 52428]
    obj = b"\0BCM2 " + struct.pack("<ffii", 10.0, 5.0, 3, 2) + struct.pack("<6H", *vals)
    want = np.array([[10.0, 15.0], [11.0, 12.0], [13.0, 14.0]])
    got = kf.read_matrix(obj)
    assert got.shape == (3, 2)
    assert np.abs(got - want).max() <= _ulp4(10.0, 5.0)


def test_cm_bytes_by_hand():
    # min_value -20, range 65.535: a uint16 v decodes to -20 + 0.001 v.  3 rows x 2 columns.
    # column 0: percentiles (0, 64, 320, 950) -> values -20 + 0.001 * (0, 64, 320, 950)
    #   b = 32  (<= 64):   0 + (64 - 0) * 32 / 64              = 32   -> -19.968
    #   b = 100 (<= 192):  64 + (320 - 64) * (100 - 64) / 128  = 136  -> -19.864
    #   b = 200 (> 192):   320 + (950 - 320) * (200 - 192) / 63 = 400 -> -19.600
    # column 1: percentiles (1000, 1640, 2920, 3550)
    #   b = 64:  1640 -> -18.360     b = 192: 2920 -> -17.080     b = 255: 3550 -> -16.450
    # the body is COLUMN-major: column 0's three bytes, then column 1's
    obj = b"\0BCM " + struct.pack("<ffii", -20.0, 65.535, 3, 2) + struct.pack("<8H", 0, 64, 320, 950, 1000, 1640, 2920, 3550) \
        + bytes([32, 100, 200, 64, 192, 255])
    want = np.array([[-19.968, -18.360], [-19.864, -17.080], [-19.600, -16.450]])
    got = kf.read_matrix(obj)
    assert got.shape == (3, 2)
    assert np.abs(got - want).max() <= _ulp4(-20.0, 65.535), (got, want)


def test_read_matrix_is_unchanged_for_plain_matrices(tmp_path):
    m = np.random.default_rng(0).standard_normal((5, 7))
    for double in (False, True):
        p = str(tmp_path / f"m{int(double)}.mat")
        kf.write_matrix_binary(p, m, double=double)
        got = kf.read_matrix(p)
        assert got.dtype == np.float64 and np.array_equal(got, m.astype("<f8" if double else "<f4").astype(np.float64))
    assert np.array_equal(kf.read_matrix(b" [\n 1 2\n 3 4 ]"), np.array([[1.0, 2.0], [3.0, 4.0]]))
    with pytest.raises(kf.KaldiFormatError):
        kf.read_matrix(b"\0BCM9 " + bytes(32))
    with pytest.raises(kf.KaldiFormatError, match="truncated"):
        kf.read_matrix(b"\0BCM3 " + struct.pack("<ffii", 0.0, 1.0, 4, 4) + bytes(15))


# ---- 2. archives and script files ---------------------------------------------------------------------------------------

def _mfcc_like(rng, T, D=30):
    x = rng.standard_normal((T, D)) * np.linspace(3.0, 0.3, D)
    x[:, 0] += 14.0
    return x


def _archive(tmp_path, n=12, D=30, seed=1):
    rng = np.random.default_rng(seed)
    fmts = ["FM", "CM", "CM2", "CM3", "DM"]
    items = [(f"utt{i:03d}", _mfcc_like(rng, int(rng.integers(1, 90)), D), fmts[i % 5]) for i in range(n)]
    ark, scp = str(tmp_path / "feats.ark"), str(tmp_path / "feats.scp")
    offs = feat_ref.write_ark(ark, items)
    order = [items[i][0] for i in rng.permutation(n)]
    feat_ref.write_scp(scp, ark, offs, order)
    return items, order, ark, scp, offs


def test_decoders_agree_with_the_restatement(tmp_path):
    items, order, ark, scp, _ = _archive(tmp_path)
    by_key = {k: (m, f) for k, m, f in items}
    n = 0
    for key, mat in kf.read_feature_ark(ark):
        ref, bound = feat_ref.decode(feat_ref.encode(*by_key[key]))
        assert mat.dtype == np.float32 and mat.shape == ref.shape
        assert np.abs(mat - ref).max() <= bound, key
        # the encoder is lossy but not absurd: a CM3 step is range / 255
        assert np.abs(ref - by_key[key][0]).max() <= (ref.max() - ref.min() + 1e-6) / 100.0 + 1e-6, key
        n += 1
    assert n == len(items)
    got = list(kf.read_feature_scp(scp))
    assert [k for k, _ in got] == order
    for key, mat in got:
        ref, bound = feat_ref.decode(feat_ref.encode(*by_key[key]))
        assert np.abs(mat - ref).max() <= bound, key


def test_load_feature_scp_descriptors_address_the_bodies(tmp_path):
    items, order, ark, scp, offs = _archive(tmp_path)
    by_key = {k: (m, f) for k, m, f in items}
    feats = kf.load_feature_scp(scp)
    keys, desc, payload = feats
    assert keys == order and feats.keys == order
    assert isinstance(payload, np.ndarray) and payload.dtype == np.uint8 and payload.ndim == 1 and payload.flags.c_contiguous
    assert desc.dtype == kf.FEAT_DESC and desc.dtype.itemsize == 40 and len(desc) == len(order)
    esz = {"FM": 4, "DM": 8, "CM": 1, "CM2": 2, "CM3": 1}
    for i, key in enumerate(order):
        mat, fmt = by_key[key]
        obj = feat_ref.encode(mat, fmt)
        d = desc[i]
        assert d["format"] == kf.FEAT_FORMATS[fmt] and d["rows"] == mat.shape[0] and d["cols"] == 30
        body = obj[len(fmt) + 1 + (10 if fmt in ("FM", "DM") else 16):]
        if fmt not in ("FM", "DM"):
            mn, rg = struct.unpack("<ff", obj[len(fmt) + 1:len(fmt) + 9])
            assert d["min_value"] == np.float32(mn) and d["range"] == np.float32(rg)
        hdr = 8 * 30 if fmt == "CM" else 0
        if hdr:
            assert payload[d["hdr_off"]:d["hdr_off"] + hdr].tobytes() == body[:hdr]
        n = esz[fmt] * mat.shape[0] * 30
        assert payload[d["data_off"]:d["data_off"] + n].tobytes() == body[hdr:] and len(body) == hdr + n
        assert d["data_off"] % esz[fmt] == 0 and feats.body(i).tobytes() == body[hdr:]
    # bounded pieces of the same scp
    part = kf.load_feature_scp(scp, entries=kf.read_scp(scp)[3:7])
    assert part.keys == order[3:7] and np.array_equal(part.desc["rows"], desc["rows"][3:7])
    # an empty scp
    empty = str(tmp_path / "empty.scp")
    open(empty, "w").close()
    e = kf.load_feature_scp(empty)
    assert e.keys == [] and len(e.desc) == 0 and e.payload.shape == (0,)


def test_truncated_archive_and_wrong_width_name_the_key(tmp_path):
    items, order, ark, scp, offs = _archive(tmp_path)
    last = items[-1][0]
    data = open(ark, "rb").read()
    cut = str(tmp_path / "cut.ark")
    with open(cut, "wb") as fh:
        fh.write(data[:-7])
    cut_scp = str(tmp_path / "cut.scp")
    feat_ref.write_scp(cut_scp, cut, offs, order)
    with pytest.raises(kf.KaldiFormatError, match=last):
        kf.load_feature_scp(cut_scp)
    with pytest.raises(kf.KaldiFormatError, match=last):
        list(kf.read_feature_scp(cut_scp))
    with pytest.raises(kf.KaldiFormatError, match=last):
        list(kf.read_feature_ark(cut))
    # a 23-column entry
    rng = np.random.default_rng(2)
    ark23, scp23 = str(tmp_path / "w.ark"), str(tmp_path / "w.scp")
    its = [("good", _mfcc_like(rng, 40), "CM"), ("narrow23", _mfcc_like(rng, 40, 23), "CM")]
    feat_ref.write_scp(scp23, ark23, feat_ref.write_ark(ark23, its), ["good", "narrow23"])
    with pytest.raises(kf.KaldiFormatError, match="narrow23"):
        kf.load_feature_scp(scp23, cols=30)
    feats = kf.load_feature_scp(scp23)  # the reader itself takes any width; the front end does not
    from neuralplda_amd import features
    with pytest.raises(ValueError, match="narrow23"):
        features.decode_features(feats, device="cuda:0")
    with pytest.raises(ValueError, match="narrow23"):
        features.prepare_features(feats, device="cuda:0")
    # an unknown token
    bad = str(tmp_path / "bad.ark")
    with open(bad, "wb") as fh:
        fh.write(b"odd \0BXM " + bytes(40))
    with open(str(tmp_path / "bad.scp"), "w") as fh:
        fh.write(f"odd {bad}:4\n")
    with pytest.raises(kf.KaldiFormatError, match="odd"):
        kf.load_feature_scp(str(tmp_path / "bad.scp"))


# ---- 3. vad.conf --------------------------------------------------------------------------------------------------------

def test_vad_options_from_conf(tmp_path):
    from neuralplda_amd import features
    import neuralplda_amd
    assert neuralplda_amd.VadOptions is features.VadOptions and neuralplda_amd.prepare_features is features.prepare_features
    assert tuple(features.VadOptions()) == (5.5, 0.5, 0.12, 2)
    p = str(tmp_path / "vad.conf")
    with open(p, "w") as fh:
        fh.write("--vad-energy-threshold=5.5\n--vad-energy-mean-scale=0.5\n--vad-proportion-threshold=0.12\n"
                 "--vad-frames-context=2\n")
    assert features.VadOptions.from_conf(p) == features.VadOptions()
    with open(p, "w") as fh:
        fh.write("# tuned\n--vad-energy-threshold=4.25  # lower\n\n--vad-frames-context=5\n")
    o = features.VadOptions.from_conf(p)
    assert o == features.VadOptions(energy_threshold=4.25, frames_context=5) and isinstance(o.frames_context, int)
    with open(p, "w") as fh:
        fh.write("--sample-frequency=8000\n")
    with pytest.raises(ValueError, match="sample-frequency"):
        features.VadOptions.from_conf(p)


# ---- 4. the C ABI and the kernels' resources --------------------------------------------------------------------------------

def test_entry_points_declared_exported_and_bound(hip_lib):
    from neuralplda_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nplda_hip.h")).read()
    nm = shutil.which("nm")
    exported = None
    if nm is not None:
        out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
        exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES, name
        assert getattr(hip_lib, name) is not None
        if exported is not None:
            assert name in exported, name
    assert hip_lib.nplda_abi_version() == 4
    assert "typedef struct nplda_feat_desc" in hdr and kf.FEAT_DESC.itemsize == 40
    # pure host arithmetic and argument checks (no device is touched)
    assert hip_lib.nplda_feat_workspace_bytes(0, 0) >= 0
    assert hip_lib.nplda_feat_workspace_bytes(1000, 10) >= (1000 + 10) * 30 * 8 + 11 * 8
    assert hip_lib.nplda_feat_decode_f32(None, 0, None, None, 0, 0, None, None) == 0      # no utterances: a no-op
    assert hip_lib.nplda_feat_cmn_select_f32(None, None, 0, 0, None, 300, 25, None, None, None, 0, None) == 0
    assert hip_lib.nplda_feat_vad_energy_f32(None, None, 0, 0, 5.5, 0.5, 0.12, 2, None, None) == 0
    assert hip_lib.nplda_feat_decode_f32(None, 0, None, None, 3, 10, None, None) == -22    # NPLDA_EINVAL


def test_new_kernels_use_no_scratch():
    from tests.test_kernel_resources_cpu import _resources
    res = _resources("nplda_feat.hip")
    for k in NEW_KERNELS:
        hit = [v for name, v in res.items() if k in name]
        assert len(hit) == 1, (k, sorted(res))
        assert hit[0]["ScratchSize"] == 0, (k, hit[0])
    assert len(res) == len(NEW_KERNELS), sorted(res)


# ---- the restatement's own rules (so that the GPU tests compare against something pinned) ------------------------------------

def test_window_rule():
    w = feat_ref.window
    assert [w(t, 1000, 300) for t in (0, 149, 150, 151, 500, 849, 850, 999)] == \
        [(0, 300), (0, 300), (0, 300), (1, 301), (350, 650), (699, 999), (700, 1000), (700, 1000)]
    assert [w(t, 10, 7) for t in (0, 3, 4, 6, 7, 9)] == [(0, 7), (0, 7), (1, 8), (3, 10), (3, 10), (3, 10)]  # 7 // 2 = 3
    assert w(0, 5, 300) == (0, 5) and w(4, 5, 300) == (0, 5) and w(0, 1, 7) == (0, 1)
    x = np.arange(24.0).reshape(12, 2)
    m = feat_ref.sliding_mean(x, 7)
    assert np.allclose(m[5], x[2:9].mean(0)) and np.allclose(m[0], x[0:7].mean(0)) and np.allclose(m[11], x[5:12].mean(0))


def test_vad_rule():
    c0 = np.array([2.0, 2.0, 2.0, 2.0, 2.0, 13.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0])
    # thr = 5.5 + 0.5 * mean = 5.5 + 0.5 * 35 / 12: only frame 5 is above; its +-2 neighbours see 1 of 5 >= 0.6
    got = feat_ref.vad_energy(c0)
    assert got.tolist() == [False] * 3 + [True] * 5 + [False] * 4
    assert feat_ref.vad_energy(np.full(9, 2.0)).sum() == 0
    assert feat_ref.vad_energy(np.full(9, 13.0)).sum() == 9   # thr = 12 < 13
    assert feat_ref.vad_energy(np.array([13.0, 2.0, 2.0, 2.0]), proportion_threshold=0.5, frames_context=1).tolist() == \
        [True, False, False, False]
