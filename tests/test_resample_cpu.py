"""The resampler without a device: the twin tests/resample_ref.py against a brute-force evaluation of the specification
(design/k29_resample.md), the output length, properties of the filter, the conditions of the inputs the GPU tests use, the
host logic of neuralplda_amd/resample.py, augment.py and tools/resample_wav_scp.py, and the resource budget of
csrc/nplda_resample.hip."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from neuralplda_amd import augment as ag, kaldi_format as kf, resample as rs
from tests import resample_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neuralplda_amd", "csrc")
NPLDA_EINVAL, NPLDA_EUNSUPPORTED = -22, -95


# ---- 1. the twin against the continuous formula ------------------------------------------------------------------------------

@pytest.mark.parametrize("rates", ref.ALL_RATES)
def test_twin_against_the_brute_force_evaluation(rates):
    """Every output sample from the continuous formula in long double, every input tried, no phase table: the phase twin on
    the unrounded table agrees to 1e-12 of the largest output (seen: 3e-16 - 5e-16); n = 300 and two short utterances."""
    rin, rout = rates
    rng = np.random.default_rng(rin + rout)
    for n in (300, ref.TAPS[rates] - 1, 1):
        x = ref.make_audio(rng, n, rin)
        want = ref.brute(x, rin, rout)
        got = ref.resample64(x, rin, rout, table32=False)
        assert got.shape == want.shape == (ref.output_length(n, rin, rout),)
        assert float(np.abs(got - want).max()) <= 1e-12 * float(np.abs(want).max()), (rates, n)


def test_bank_of_the_module_is_the_twins_and_has_the_stated_sizes():
    for rates in ref.ALL_RATES + ((15200, 16000), (16800, 16000), (48000, 8000)):
        iu, ou, first, w, counts = ref.filter_bank(*rates)
        iu2, ou2, first2, w2 = rs.filter_bank(*rates)
        assert (iu, ou) == (iu2, ou2) == ref.units(*rates) and np.array_equal(first, first2) and w.shape == w2.shape
        assert np.abs(w - w2).max() <= 1e-15 * np.abs(w).max()
        assert w.shape[1] == counts.max() <= rs.MAX_TAPS and max(iu, ou) <= rs.MAX_UNITS
        if rates in ref.TAPS:
            assert w.shape[1] == ref.TAPS[rates], rates
        # what the kernel relies on: the first input of an output does not decrease with the output
        assert (np.diff(first) >= 0).all() and first[-1] <= first[0] + iu


# ---- 2. the output length --------------------------------------------------------------------------------------------------------

def test_output_length_against_a_direct_count():
    for rin, rout in ref.ALL_RATES:
        iu, ou = ref.units(rin, rout)
        for n in range(51):
            count = sum(1 for k in range(n * ou + 1) if k * iu < n * ou)
            assert ref.output_length(n, rin, rout) == count == -(-(rout * n) // rin), (rin, rout, n)
        assert np.array_equal(rs.output_lengths(np.arange(51), rin, rout), [ref.output_length(n, rin, rout) for n in range(51)])
    assert rs.output_lengths([10, 10, 0], [16000, 8000, 44100], [8000, 16000, 16000]).tolist() == [5, 20, 0]


# ---- 3. sanity of the filter -----------------------------------------------------------------------------------------------------

def test_phase_sums_and_a_tone():
    """Every phase's weights sum to within 1e-3 of 1 (seen: 1.00004 - 1.00088); a 1 kHz tone of amplitude 10 000 comes out as
    the 1 kHz tone at the new rate within 0.2 % of the amplitude away from the edges (seen: at most 0.087 %)."""
    worst = 0.0
    for rin, rout in ref.ALL_RATES:
        iu, ou, first, w, _ = ref.filter_bank(rin, rout)
        assert np.abs(w.sum(axis=1) - 1.0).max() < 1e-3, (rin, rout)
        n = rin // 4
        x = 10000.0 * np.sin(2.0 * np.pi * 1000.0 * np.arange(n) / rin + 0.3)
        y = ref.resample64(x, rin, rout, table32=False)
        k = np.arange(len(y))
        edge = 2 * w.shape[1]
        err = np.abs(y - 10000.0 * np.sin(2.0 * np.pi * 1000.0 * k / rout + 0.3))[edge:-edge].max()
        worst = max(worst, err / 10000.0)
        assert err <= 0.002 * 10000.0, (rin, rout, err)
    print(f"tone: worst relative error {100 * worst:.3f} %")


# ---- 4. the conditions of the GPU tests' inputs ----------------------------------------------------------------------------------

def test_conditions_of_the_gpu_cases():
    assert ref.CHUNK == rs.CHUNK
    cases = ref.grid_case()
    assert len(cases) == 42
    for rin, rout in ref.RATES:
        taps = rs.filter_bank(rin, rout)[3].shape[1]
        ns = ref.grid_lengths(rin, rout)
        assert ns[:4] == (1, 2, taps - 1, taps)
        # one input sample less fills at most the first chunk, one more opens the second
        assert ref.output_length(ns[4], rin, rout) <= ref.CHUNK < ref.output_length(ns[5], rin, rout)
        assert ns[5] - ns[4] == 2
    assert max(ref.output_length(5000, a, b) for a, b in ref.RATES) > 4 * ref.CHUNK
    mixed = ref.mixed_case()
    assert len({(a, b) for _, a, b in mixed if a != b}) == 9
    for x, _, _ in cases + mixed:
        assert x.dtype == np.int16


def test_condition_of_the_16_bit_cap():
    """The GPU test allows the kernel 0.5 % of samples that differ from rint(resample64) per case of 20 000; the float32 twin
    alone, whose chain of separate multiplies and adds has the larger rounding error (|error| ~ 1e-3: a sample differs when
    its value lies that close to a half), must stay under half the cap.  Seen: 0.000 - 0.055 %."""
    for x, rin, rout in ref.big_cases():
        a, _ = ref.round_int16(ref.resample64(x, rin, rout))
        b, _ = ref.round_int16(ref.resample32(x, rin, rout))
        d = np.abs(a.astype(np.int64) - b)
        print(f"{rin}->{rout}: {100 * (d > 0).mean():.4f} %")
        assert d.max() <= 1 and (d > 0).mean() <= 0.0025, (rin, rout, float((d > 0).mean()))
        assert len(x) == 20000


# ---- 5. host logic ---------------------------------------------------------------------------------------------------------------

def _call(**kw):
    c = rs._Call()
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_status_codes_before_anything_is_enqueued(hip_lib):
    lib = hip_lib
    run = lambda c: lib.nplda_resample_batch(ctypes.addressof(c), None)   # noqa: E731
    assert lib.nplda_resample_batch(None, None) == NPLDA_EINVAL
    assert run(_call(n_utts=0)) == 0                                              # a no-op, whatever else it holds
    assert run(_call(n_utts=-1)) == NPLDA_EINVAL
    ok = dict(n_utts=1, n_ratios=1, total_chunks=1, max_iu=9, max_ou=10, max_taps=13, max_span=1024)
    for over in (dict(max_iu=1025), dict(max_ou=1025), dict(max_taps=129), dict(max_span=16385), dict(n_utts=1 << 31),
                 dict(total_chunks=1 << 31)):
        assert run(_call(**{**ok, **over})) == NPLDA_EUNSUPPORTED, over
    for bad in (dict(max_iu=0), dict(max_ou=-1), dict(max_taps=0), dict(max_span=0), dict()):   # the last: null pointers
        assert run(_call(**{**ok, **bad})) == NPLDA_EINVAL, bad
    assert lib.nplda_resample_chunk() == rs.CHUNK
    assert lib.nplda_resample_span_floats(441, 80, 67) * 4 <= 65536
    assert lib.nplda_resample_span_floats(1025, 1, 13) == 0 and lib.nplda_resample_span_floats(1, 1, 129) == 0
    for iu, ou, taps in ((9, 10, 13), (441, 80, 67), (1024, 97, 128), (1, 1024, 13)):
        assert lib.nplda_resample_span_floats(iu, ou, taps) >= (rs.CHUNK - 1) * iu // ou + 1 + taps + 7
    # the chunk table (csrc/nplda_ragged.h's walk): utterance and chunk of the utterance, empty utterances stepped over
    offs = np.array([0, 1, 1, 1 + 1024, 1 + 1024 + 2049], dtype=np.int64)
    assert lib.nplda_resample_chunk_table(offs.ctypes.data, 4, None, 0) == 5
    table = np.zeros((5, 2), np.int32)
    assert lib.nplda_resample_chunk_table(offs.ctypes.data, 4, table.ctypes.data, 5) == 5
    assert table.tolist() == [[0, 0], [2, 0], [3, 0], [3, 1], [3, 2]]
    assert lib.nplda_resample_chunk_table(offs.ctypes.data, 4, table.ctypes.data, 4) == -28          # NPLDA_ENOSPC
    bad = np.array([0, 5, 3], dtype=np.int64)
    assert lib.nplda_resample_chunk_table(bad.ctypes.data, 2, None, 0) == NPLDA_EINVAL
    assert lib.nplda_abi_version() == 4


def test_value_errors_name_the_argument(hip_lib):
    x = np.zeros(100, np.int16)
    cases = [
        (dict(rate_in=0, rate_out=16000), "rate_in"),
        (dict(rate_in=16000, rate_out=-8000), "rate_out"),
        (dict(rate_in=[16000, 16000.5], rate_out=8000), "utterance 1: rate_in"),
        (dict(rate_in=[8000, 16001], rate_out=16000), "utterance 1: .*16001:16000"),          # ou beyond the limit
        (dict(rate_in=[8000, 16000 * 11], rate_out=16000), "utterance 1: .*taps"),             # 11:1 takes 134 taps
        (dict(rate_in=8000, rate_out=16000, gain=[1.0, np.nan]), "utterance 1: gain"),
        (dict(rate_in=[8000] * 3, rate_out=16000), "rate_in: expected a scalar or one value per utterance"),
    ]
    for kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            rs.prepare(x, [0, 50, 100], **kw)
    for offs in ([0, 60, 50], [0, 50, 101], [-1, 50, 100], []):
        with pytest.raises(ValueError, match="offsets"):
            rs.prepare(x, offs, 8000, 16000)
    with pytest.raises(ValueError, match="int16"):
        rs.prepare(x.astype(np.float32), [0, 50, 100], 8000, 16000)
    with pytest.raises(ValueError, match="out_dtype"):
        rs.prepare(x, [0, 50, 100], 8000, 16000, out_dtype=np.float64)
    with pytest.raises(ValueError, match="speed factor"):
        rs.speed_perturb(x, [0, 50, 100], [0.9, 0.0], 16000)
    with pytest.raises(ValueError, match="rate_in"):
        rs.filter_bank(0, 16000)
    assert rs.speed_rates([0.9, 1.0, 1.1], 16000).tolist() == [14400, 16000, 17600]
    assert rs.filter_bank(16000 * 11, 16000)[3].shape[1] > rs.MAX_TAPS


class _Noises:
    sample_frequency = 16000.0
    lengths = np.array([3000, 8000, 12000, 500], dtype=np.int64)

    def __len__(self):
        return 4

    def items_of(self, kind):
        return np.arange(4, dtype=np.int64)


class _Rirs:
    sample_frequency = 16000.0

    def __len__(self):
        return 3


def _same(a, b):
    return (np.array_equal(a.rir, b.rir) and a.additive == b.additive and np.array_equal(a.speed, b.speed)
            and np.array_equal(a.shift_output, b.shift_output) and np.array_equal(a.volume, b.volume))


def test_augmenter_speeds_and_recipe_speed():
    lengths = np.random.default_rng(2).integers(1, 60000, 40)
    for seed in (0, 8):
        plain = ag.Augmenter(_Rirs(), _Noises(), seed=seed).draw(lengths)
        none = ag.Augmenter(_Rirs(), _Noises(), seed=seed, speeds=None).draw(lengths)
        assert _same(plain, none) and (plain.speed == 1.0).all()                   # no draw is added
        whole = ag.Augmenter(_Rirs(), _Noises(), seed=seed, speeds=(0.9, 1.0, 1.1)).draw(lengths)
        halves = ag.Augmenter(_Rirs(), _Noises(), seed=seed, speeds=(0.9, 1.0, 1.1))
        a, b = halves.draw(lengths[:17]), halves.draw(lengths[17:])
        assert np.array_equal(np.concatenate([a.speed, b.speed]), whole.speed) and a.additive + b.additive == whole.additive
        assert np.array_equal(np.concatenate([a.rir, b.rir]), whole.rir)
        assert set(whole.speed.tolist()) == {0.9, 1.0, 1.1} and not _same(whole, plain)
        # the foreground noises are laid out over the PERTURBED length
        n2 = ag.perturbed_lengths(lengths, whole, 16000)
        assert np.array_equal(n2, [ref.output_length(n, round(f * 16000), 16000) for n, f in zip(lengths, whole.speed)])
        fg = [(u, e) for u, e in enumerate(whole.additive) if e and not e[0][3]]
        assert fg and all(e[-1][1] < n2[u] for u, e in fg)
    # 16 000 samples at half speed are 32 000: a second foreground noise (items of 500 samples, a second apart) fits
    class Short(_Noises):
        lengths = np.full(4, 500, dtype=np.int64)
    slow = ag.Augmenter(None, Short(), kinds=("noise",), speeds=(0.5,)).draw([16000])
    assert [e[1] for e in slow.additive[0]] == [0, 16500] and slow.speed.tolist() == [0.5]
    assert [e[1] for e in ag.Augmenter(None, Short(), kinds=("noise",)).draw([16000]).additive[0]] == [0]
    rec = ag.Recipe([0, -1, 1], speed=[0.9, 1.0, 1.1], volume=[0.0, 0.5, 0.0])
    sel = rec.select([2, 0])
    assert sel.speed.tolist() == [1.1, 0.9] and sel.rir.tolist() == [1, 0]
    assert rec.at_unit_speed().speed.tolist() == [1.0] * 3 and rec.at_unit_speed().volume.tolist() == [0.0, 0.5, 0.0]
    assert ag.Recipe([0, -1]).speed.tolist() == [1.0, 1.0] and ag.Recipe.clean(2).speed.tolist() == [1.0, 1.0]
    assert ag.output_lengths([1000, 1000, 1000], ag.Recipe([-1] * 3, speed=[0.9, 1.0, 1.1]), None, 16000).tolist() == [1112, 1000, 910]
    with pytest.raises(ValueError, match="sample_frequency"):
        ag.output_lengths([1000], ag.Recipe([-1], speed=0.9), None)
    with pytest.raises(ValueError, match="utterance 1: speed"):
        ag.Recipe([-1, -1], speed=[1.0, 0.0]).validate([5, 5], None, None)
    ag.Augmenter(_Rirs(), _Noises(), speeds=(0.999,))                            # 15984:16000 = 999:1000: within the limits
    with pytest.raises(ValueError, match="speed 0.9999.*7999:8000"):             # 15998:16000: beyond the 1024 phases
        ag.Augmenter(_Rirs(), _Noises(), speeds=(0.9999,))


def test_load_wav_scp_returns_the_rates(tmp_path):
    rng = np.random.default_rng(4)
    scp = str(tmp_path / "wav.scp")
    with open(scp, "w") as fh:
        for i, (n, r) in enumerate(((300, 8000), (500, 16000))):
            p = str(tmp_path / f"u{i}.wav")
            kf.write_wav(p, ref.make_audio(rng, n, r), r)
            fh.write(f"u{i} {p}\n")
    keys, offsets, samples, rates = kf.load_wav_scp(scp, return_rates=True)
    assert keys == ["u0", "u1"] and offsets.tolist() == [0, 300, 800] and rates.tolist() == [8000, 16000] and rates.dtype == np.int64
    assert len(kf.load_wav_scp(scp)) == 3
    with pytest.raises(kf.KaldiFormatError, match="there is no resampling"):
        kf.load_wav_scp(scp, sample_frequency=16000, return_rates=True)
    for table in (ag.NoiseTable, ag.RirTable):
        with pytest.raises(ValueError, match="sample rate 8000, expected 16000"):
            table([str(tmp_path / "u0.wav")], 16000)


def test_tool_names_the_copies_as_kaldi_does(tmp_path):
    spec = importlib.util.spec_from_file_location("resample_wav_scp", os.path.join(ROOT, "tools", "resample_wav_scp.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rng = np.random.default_rng(5)
    for k in ("spkA-utt1", "spkB-utt1"):
        kf.write_wav(str(tmp_path / f"{k}.wav"), ref.make_audio(rng, 200), 16000)
    u2s_path = str(tmp_path / "utt2spk")
    with open(u2s_path, "w") as fh:
        fh.write("spkA-utt1 spkA\nspkB-utt1 spkB\n")
    u2s = tool.read_utt2spk(u2s_path)
    copies, new = tool.plan_copies(["spkA-utt1", "spkB-utt1"], ["0.9", "1.0", "1.1"], u2s)
    assert [c[0] for c in copies] == ["sp0.9-spkA-utt1", "sp0.9-spkB-utt1", "sp1.0-spkA-utt1", "sp1.0-spkB-utt1",
                                      "sp1.1-spkA-utt1", "sp1.1-spkB-utt1"]
    assert copies[0] == ("sp0.9-spkA-utt1", "spkA-utt1", "0.9")
    assert new["sp1.1-spkB-utt1"] == "sp1.1-spkB" and len(new) == 6
    out = tmp_path / "out"
    out.mkdir()
    tool.write_tables(str(out), copies, new)
    assert (out / "utt2spk").read_text().splitlines()[0] == "sp0.9-spkA-utt1 sp0.9-spkA"
    assert (out / "spk2utt").read_text().splitlines() == [f"sp{f}-spk{s} sp{f}-spk{s}-utt1" for f in ("0.9", "1.0", "1.1")
                                                          for s in "AB"]
    scp = kf.read_scp(str(out / "wav.scp"))
    assert [k for k, _ in scp] == [c[0] for c in copies] and scp[0][1].endswith("sp0.9-spkA-utt1.wav")
    plain, none = tool.plan_copies(["b", "a"])
    assert plain == [("a", "a", None), ("b", "b", None)] and none is None
    with pytest.raises(ValueError, match="distinct"):
        tool.plan_copies(["a"], ["0.9", "0.9"])


# ---- 6. the kernel's resources ---------------------------------------------------------------------------------------------------

def test_register_and_lds_budget_of_the_resample_kernels():
    """design/k29_resample.md: no scratch, no static LDS (the span is dynamic, at most 64 KB a block), and at most 64
    registers (the compiler reports 44): eight blocks of four waves per CU wherever their spans fit its 160 KB of LDS (the kernel is bound by the
    latency of a block's chain of loads, which only more resident blocks hide)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    err = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                          "-c", os.path.join(CSRC, "nplda_resample.hip"), "-o", os.devnull,
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900).stderr
    res, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"remark: +(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"LDS Size \[bytes/block\]): +(\S+)", line)
        if m and m.group(1) == "Function Name":
            cur = res.setdefault(m.group(2), {})
        elif m and cur is not None:
            cur[m.group(1).split(" ")[0]] = int(m.group(2))
    main = {k: v for k, v in res.items() if "rs_kernel" in k}
    assert len(main) == 2 and len(res) == 3, sorted(res)      # int16 and float32 output, and the clear kernel
    for name, v in res.items():
        assert v["ScratchSize"] == 0 and v["LDS"] == 0 and v["AGPRs"] == 0, (name, v)
    for name, v in main.items():
        assert v["VGPRs"] <= 64 and v["Occupancy"] >= 8, (name, v)
