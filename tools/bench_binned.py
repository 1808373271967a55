"""probabilit_amd.inspection's conditional statistics against their yardsticks, at the same size:

    pbh_binned_sums alone (the C call between two events, buffers allocated before): 1, 15 and 32
        inputs binned against one output, 32 and 1024 bins, uniform and quantile edges
    pbh_hbm_copy                                                            the HBM yardstick
    pbh_histogram2d alone on the same columns, the same pairs and as many bins per binning axis: the
        same bytes and the same lookup, so the difference is the price of the two FP64 LDS adds per row
        (it takes at most 16 columns: 15 pairs stand beside the 32)
    sensitivity(output, *32 inputs) end to end
    two columns' download + scipy.stats.binned_statistic on the host       the existing route

Device figures are times between two HIP events on the launching stream (torch.cuda.Event on the
current stream) after warm-up calls, the median over the repetitions.  The kernel reads 16 B per
row per pair; its ceiling is that many bytes at the measured copy rate.  The host route is wall
time, once: the download of two whole columns, and binned_statistic on the first --host-rows rows
scaled to n (stated in the JSON).

    python tools/bench_binned.py [--n 100000000] [--reps 20] [--warmup 3] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
import probabilit_amd  # noqa: E402,F401
from probabilit_amd import _lib, device, inspection  # noqa: E402
from probabilit_amd.modeling import Distribution  # noqa: E402

from bench_joint import timed  # noqa: E402


def binned_call(cols, edges, uniform):
    """A closure that enqueues pbh_binned_sums of (input c, output 0) for every input and nothing
    else.  cols[0] is the output (no bins)."""
    lib = _lib.load()
    k, n = len(cols), cols[0].shape[0]
    bins = np.array([0] + [len(e) - 1 for e in edges], dtype=np.int32)
    uni = np.array([0] + [int(uniform)] * (k - 1), dtype=np.uint8)
    flat = np.concatenate(edges)
    ptrs = np.array([x.data_ptr() for x in cols], dtype=np.uint64)
    centres = np.zeros(k)
    centres[0] = inspection._moment_rows(cols[0])[0]["mean"]
    pairs = np.array([(c, 0) for c in range(1, k)], dtype=np.int32)
    b = ctypes.c_size_t()
    _lib.check(lib.pbh_binned_sums_workspace_size(k, _lib.np_ptr(bins), ctypes.byref(b)))
    ws = device.empty(b.value, "uint8")
    total = int(bins.sum())
    counts, s1, s2 = device.empty(total, "int64"), device.empty(total), device.empty(total)
    keep = (bins, uni, flat, ptrs, centres, pairs, ws, counts, s1, s2)

    def call():
        _lib.check(lib.pbh_binned_sums(_lib.np_ptr(ptrs), k, n, _lib.np_ptr(flat), _lib.np_ptr(bins), _lib.np_ptr(uni),
                                       _lib.np_ptr(centres), _lib.np_ptr(pairs), len(pairs), counts.data_ptr(),
                                       s1.data_ptr(), s2.data_ptr(), ws.data_ptr(), b.value, device.stream()),
                   "pbh_binned_sums")

    call.keep, call.pairs, call.counts = keep, len(pairs), counts
    return call


def joint_call(cols, edges):
    """pbh_histogram2d of (input c, output 0) for every input; edges[0] is the output's."""
    lib = _lib.load()
    k, n = len(cols), cols[0].shape[0]
    bins = np.array([len(e) - 1 for e in edges], dtype=np.int32)
    uniform = np.ones(k, dtype=np.uint8)
    flat = np.concatenate(edges)
    ptrs = np.array([x.data_ptr() for x in cols], dtype=np.uint64)
    pairs = np.array([(c, 0) for c in range(1, k)], dtype=np.int32)
    b = ctypes.c_size_t()
    _lib.check(lib.pbh_histogram2d_workspace_size(k, _lib.np_ptr(bins), ctypes.byref(b)))
    ws = device.empty(b.value, "uint8")
    counts = device.empty(int(sum(bins[i] * bins[j] for i, j in pairs)), "int64")
    keep = (bins, uniform, flat, ptrs, pairs, ws, counts)

    def call():
        _lib.check(lib.pbh_histogram2d(_lib.np_ptr(ptrs), k, n, _lib.np_ptr(flat), _lib.np_ptr(bins),
                                       _lib.np_ptr(uniform), _lib.np_ptr(pairs), len(pairs), counts.data_ptr(),
                                       ws.data_ptr(), b.value, device.stream()), "pbh_histogram2d")

    call.keep, call.pairs, call.counts = keep, len(pairs), counts
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inputs", type=int, default=32)
    ap.add_argument("--host-rows", type=int, default=10_000_000)
    ap.add_argument("--out", default="profiles/binned/bench_binned.json")
    a = ap.parse_args()
    import torch

    n, K = a.n, a.inputs
    xs = [Distribution("norm", loc=0.1 * c, scale=1.0 + 0.05 * c) for c in range(K)]
    y = xs[0] * xs[1] + 2.0 * xs[2]
    for x in xs[3:]:
        y = y + 0.1 * x
    y.sample_device(n, random_state=0)
    cols = [y.samples_device] + [x.samples_device for x in xs]
    nbytes = 8 * n
    res = {"rows": n, "column_bytes": nbytes, "inputs": K, "reps": a.reps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(device.device()), "timer": "HIP events on the launching stream",
           "cases": {}}
    cases = res["cases"]

    dst = device.empty(n)
    lib = _lib.load()
    copies = {}
    for variant in range(5):
        copies[variant] = timed(lambda: _lib.check(lib.pbh_hbm_copy(cols[0].data_ptr(), dst.data_ptr(), nbytes, variant,
                                                                    device.stream())), a.reps, a.warmup)
    best = min(copies, key=lambda v: copies[v]["median_ms"])
    copy_rate = 2 * nbytes / (copies[best]["median_ms"] * 1e-3)  # a copy moves 2 bytes per byte of the vector
    cases["pbh_hbm_copy"] = dict(copies[best], variant=best, bytes_moved=2 * nbytes,
                                 tb_per_s=round(copy_rate / 1e12, 3))
    del dst

    moms = [inspection._moment_rows(x)[0] for x in cols]

    def uniform_edges(c, bins):
        return np.linspace(moms[c]["min"], moms[c]["max"], bins + 1)

    def quantile_edges(c, bins):
        ranks = inspection.quantile_ranks(n, bins)
        got, _ = inspection._select(cols[c], ranks)
        return inspection.quantile_edges([got[r] for r in ranks.tolist()])

    def report(name, call, r, extra):
        r.update(extra)
        r["pairs"] = call.pairs
        r["bytes_read"] = 16 * n * call.pairs
        rate = r["bytes_read"] / (r["median_ms"] * 1e-3)
        r["tb_per_s"] = round(rate / 1e12, 3)
        r["copy_of_the_same_bytes_ms"] = round(r["bytes_read"] / copy_rate * 1e3, 4)
        r["fraction_of_copy_rate"] = round(rate / copy_rate, 3)
        r["counted_rows_per_pair"] = int(device.to_host(call.counts).sum()) // call.pairs
        cases[name] = r
        print(name, json.dumps({k_: r[k_] for k_ in ("median_ms", "tb_per_s", "fraction_of_copy_rate")}), flush=True)

    def binned_case(name, inputs, bins, kind):
        make = uniform_edges if kind == "uniform" else quantile_edges
        call = binned_call(cols[:1 + inputs], [make(c, bins) for c in range(1, 1 + inputs)], kind == "uniform")
        report(name, call, timed(call, a.reps, a.warmup), {"bins": bins, "edges": kind})

    def joint_case(name, inputs, bins, out_bins):
        edges = [uniform_edges(0, out_bins)] + [uniform_edges(c, bins) for c in range(1, 1 + inputs)]
        call = joint_call(cols[:1 + inputs], edges)
        report(name, call, timed(call, a.reps, a.warmup), {"bins": [bins, out_bins], "edges": "uniform"})

    few = min(15, K)  # (pbh_histogram2d takes 16 columns)
    binned_case("pbh_binned_sums_1_pair_32_bins_uniform", 1, 32, "uniform")
    binned_case("pbh_binned_sums_1_pair_32_bins_quantile", 1, 32, "quantile")
    binned_case(f"pbh_binned_sums_{few}_pairs_32_bins_uniform", few, 32, "uniform")
    binned_case(f"pbh_binned_sums_{K}_pairs_32_bins_uniform", K, 32, "uniform")
    binned_case(f"pbh_binned_sums_{K}_pairs_32_bins_quantile", K, 32, "quantile")
    binned_case("pbh_binned_sums_1_pair_1024_bins_uniform", 1, 1024, "uniform")
    binned_case("pbh_binned_sums_1_pair_1024_bins_quantile", 1, 1024, "quantile")
    joint_case("pbh_histogram2d_1_pair_32x32", 1, 32, 32)
    joint_case(f"pbh_histogram2d_{few}_pairs_32x32", few, 32, 32)
    joint_case("pbh_histogram2d_1_pair_1024x16", 1, 1024, 16)

    name = f"sensitivity_{K}_inputs_32_bins"
    for binning in ("quantile", "uniform"):
        cases[f"{name}_{binning}"] = timed(lambda: inspection.sensitivity(y, *xs, bins=32, binning=binning),
                                           max(a.reps // 4, 1), 1)
        print(name, binning, cases[f"{name}_{binning}"]["median_ms"], "ms", flush=True)
    cases["binned_statistic_mean_32_bins"] = timed(lambda: inspection.binned_statistic(xs[0], y, "mean", bins=32),
                                                   a.reps, a.warmup)
    s = inspection.sensitivity(y, *xs, bins=32)
    res["first_order"] = {"largest": [int(i) for i in s.order()[:3]],
                          "eta2": [round(float(v), 4) for v in s.first_order[s.order()[:3]]]}
    assert all(d.__dict__.get("_host") is None for d in xs + [y])

    # the existing route, once: two downloads through the pinned ring, then scipy on the host
    import scipy.stats

    device.synchronize()
    t0 = time.perf_counter()
    hx, hy = xs[0].samples_, y.samples_
    t1 = time.perf_counter()
    m = min(a.host_rows, n)
    scipy.stats.binned_statistic(hx[:m], hy[:m], "mean", bins=32)
    t2 = time.perf_counter()
    cases["host_route"] = {"download_2_columns_ms": round((t1 - t0) * 1e3, 1), "scipy_binned_statistic_rows": m,
                           "scipy_binned_statistic_ms_measured": round((t2 - t1) * 1e3, 1),
                           "scipy_binned_statistic_ms_scaled_to_n": round((t2 - t1) * 1e3 * n / m, 1),
                           "scaled": m != n, "per": "one input; the download of all columns and one call per input "
                           "scale both figures by the number of inputs", "timer": "wall clock, one run"}
    print("host_route", json.dumps(cases["host_route"]), flush=True)

    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
