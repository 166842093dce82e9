#!/usr/bin/env python3
"""Cost of estimating the LDA / PLDA initialisation from x-vectors (neuralplda_amd/backend.py).

    python tools/bench_backend.py [--rows 1200000] [--dim 512] [--speakers 7323] [--lda-dim 150] [--reps 7] [--json FILE]

Seeded synthetic x-vectors (a mean, a speaker offset and noise; speaker sizes from a seeded draw, every speaker >= 1 row):

  (a) scatter: nplda_class_scatter_f32 — sum, scatter and per-speaker sums about a pivot, one call (five launches)   device events
  (b) torch:   the same statistics through the library: x.T @ x in fp32 plus index_add_ of the rows                  device events
  (c) fit:     backend.fit_backend end to end (class layout, both statistics passes, projection, EM, host algebra)   host clock + sync

Every figure is the median of --reps runs after one warm-up, with the minimum and maximum next to it.  (a) is set against the
fp32 matrix peak counting N n (n + 1) FLOP (the symmetric half) and against the time 4 N n bytes take at the HBM peak; the
bytes the call really moves are NOT measured here (that takes a counter run): the tiling's own count of table passes is
printed instead, named as a model.  Nothing is gated: design/k15_backend_estimation.md records the numbers."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_features import dev_timed, stats  # noqa: E402

PEAK_FP32_MFMA = 157.3e12
PEAK_HBM = 8.0e12


class DeviceTable:
    """What fit_backend needs of an XvectorTable — `row_of` and `on()` — over a tensor that was made on the device."""

    def __init__(self, ids, x):
        self.ids, self.x = ids, x
        self.row_of = {u: i for i, u in enumerate(ids)}

    def on(self, device):
        return self.x


def synth(N, D, S, dev, seed=0):
    rng = np.random.default_rng(seed)
    w = rng.gamma(2.0, size=S)
    sizes = rng.multinomial(N - S, w / w.sum()) + 1
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    g = torch.Generator(device=dev).manual_seed(seed)
    spk = torch.repeat_interleave(torch.arange(S, device=dev), torch.from_numpy(sizes).to(dev))
    x = torch.randn((N, D), generator=g, device=dev, dtype=torch.float32)
    h = torch.randn((S, D), generator=g, device=dev, dtype=torch.float32)
    x += h[spk]
    x += 0.5
    return x, offs, spk


def table_passes(n, tile=128):
    """Table passes the scatter kernel's block tiles ask of the cache hierarchy (a model, not a measurement): an
    off-diagonal block tile reads two column panels, a diagonal one reads one."""
    T = (n + tile - 1) // tile
    return (T * tile + T * (T - 1) // 2 * 2 * tile) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_200_000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--speakers", type=int, default=7323)
    ap.add_argument("--lda-dim", type=int, default=150)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_backend.py measures on a HIP device; none is visible")
    from neuralplda_amd import _lib, backend, ops
    dev = torch.device("cuda:0")
    lib = _lib.load()
    N, n, S = a.rows, a.dim, a.speakers
    x, offs, spk = synth(N, n, S, dev)
    offs_d = torch.from_numpy(offs).to(dev)
    res = {"gpu": torch.cuda.get_device_name(dev), "rows": N, "dim": n, "speakers": S, "lda_dim": a.lda_dim,
           "flop_counted": N * n * (n + 1), "algorithmic_bytes": 4 * N * n,
           "command": " ".join(["python", "tools/bench_backend.py"] + sys.argv[1:])}

    pivot = x[::max(1, N // 4096)][:4096].mean(0).contiguous()
    sm = torch.empty(n, dtype=torch.float64, device=dev)
    sc = torch.empty((n, n), dtype=torch.float64, device=dev)
    cs = torch.empty((S, n), dtype=torch.float64, device=dev)
    nbytes = lib.nplda_class_scatter_workspace_bytes(N, S, n)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    st = _lib.current_stream(dev)

    def k_scatter():
        _lib.check(lib.nplda_class_scatter_f32(x.data_ptr(), N, x.stride(0), None, N, offs_d.data_ptr(), S, n, pivot.data_ptr(),
                                               sm.data_ptr(), sc.data_ptr(), cs.data_ptr(), 0, ws.data_ptr(), nbytes, st),
                   "nplda_class_scatter_f32")
    r = res["a_class_scatter_call"] = dev_timed(k_scatter, dev, a.reps)
    t = r["median_s"]
    r["workspace_bytes"] = int(nbytes)
    r["tflops_counted"] = res["flop_counted"] / t / 1e12
    r["fraction_of_fp32_matrix_peak"] = res["flop_counted"] / t / PEAK_FP32_MFMA
    r["bound"] = "matrix pipe (%.2f ms at peak; 4 N n bytes take %.2f ms at the HBM peak)" % (
        res["flop_counted"] / PEAK_FP32_MFMA * 1e3, res["algorithmic_bytes"] / PEAK_HBM * 1e3)
    r["hbm_bytes_over_algorithmic"] = "not measured"
    r["modelled_table_passes"] = table_passes(n) + 1.0   # + the class-sum kernel's pass

    def k_torch():
        g = x.T @ x
        c = torch.zeros((S, n), dtype=torch.float32, device=dev).index_add_(0, spk, x)
        return g, c
    r = res["b_torch_same_statistics"] = dev_timed(k_torch, dev, a.reps)
    r["tflops_counted"] = res["flop_counted"] / r["median_s"] / 1e12
    res["a_over_b"] = t / r["median_s"]
    # what fp32 without a pivot costs in accuracy next to the kernel, on the scatter's diagonal (fp64 on a sample of columns)
    g32, _ = k_torch()
    cols = torch.arange(0, n, max(1, n // 16), device=dev)
    exact = (x[:, cols].double() ** 2).sum(0)
    mine = sc.diagonal()[cols] + 2 * pivot.double()[cols] * sm[cols] + N * pivot.double()[cols] ** 2
    res["diag_rel_err"] = {"kernel": float(((mine - exact).abs() / exact).max()),
                           "torch_fp32": float(((g32.diagonal()[cols].double() - exact).abs() / exact).max())}
    del g32

    ids = [f"u{i}" for i in range(N)]
    table = DeviceTable(ids, x)
    spk2utt = [(f"s{s}", ids[offs[s]:offs[s + 1]]) for s in range(S)]
    times = []
    for i in range(max(2, a.reps // 2) + 1):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        be = backend.fit_backend(table, spk2utt, a.lda_dim, device=dev)
        torch.cuda.synchronize(dev)
        if i:
            times.append(time.perf_counter() - t0)
    res["c_fit_backend"] = stats(times)
    res["c_fit_backend"]["psi_first_last"] = [float(be.psi[0]), float(be.psi[-1])]
    t0 = time.perf_counter()
    backend.class_layout(table, spk2utt)
    res["c_fit_backend"]["of_which_class_layout_s"] = time.perf_counter() - t0
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    with torch.no_grad():
        sys.exit(main())
