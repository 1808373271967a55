"""probabilit_amd.inspection's joint histograms against the route they replace, at the same size:

    histogram2d(a, b, bins=64) of two correlated norm nodes, pairgrid of 4 and of 8 nodes    on the device
    pbh_histogram2d alone for each (the C call between two events, buffers allocated before)
    pbh_hbm_copy                                                                             the HBM yardstick
    both columns' download + np.histogram2d on the host                                      the existing route

Device figures are times between two HIP events on the launching stream (torch.cuda.Event on the
current stream) after warm-up calls, the median over the repetitions.  The kernel reads 16 B per
row per pair; its ceiling is that many bytes at the measured copy rate (for one pair the copy of
one column moves exactly those bytes).  The host route is wall time, once: the download of both
whole columns, and np.histogram2d on the first --host-rows rows scaled to n (stated in the JSON).

    python tools/bench_joint.py [--n 100000000] [--reps 20] [--warmup 3] [--out FILE]
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
from probabilit_amd.modeling import Distribution, NoOp  # noqa: E402


def timed(fn, reps, warmup):
    import torch

    for _ in range(warmup):
        fn()
    device.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "reps_ms": [round(m, 4) for m in ms]}


def c_call(cols, edges):
    """A closure that enqueues pbh_histogram2d of every pair i < j of `cols` and nothing else."""
    lib = _lib.load()
    k, n = len(cols), cols[0].shape[0]
    bins = np.array([len(e) - 1 for e in edges], dtype=np.int32)
    uniform = np.ones(k, dtype=np.uint8)
    flat = np.concatenate(edges)
    ptrs = np.array([x.data_ptr() for x in cols], dtype=np.uint64)
    pairs = np.array([(i, j) for i in range(k) for j in range(i + 1, k)], dtype=np.int32)
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
    ap.add_argument("--host-rows", type=int, default=10_000_000)
    ap.add_argument("--out", default="profiles/joint/bench_joint.json")
    a = ap.parse_args()
    import torch

    n = a.n
    ds = [Distribution("norm", loc=0.5 * c, scale=1.0 + 0.25 * c) for c in range(8)]
    root = NoOp(*ds).correlate(ds[0], ds[1], corr_mat=np.array([[1.0, 0.8], [0.8, 1.0]]))
    root.sample_device(n, random_state=0)
    cols = [d.samples_device for d in ds]
    nbytes = 8 * n
    res = {"rows": n, "column_bytes": nbytes, "reps": a.reps, "warmup": a.warmup,
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
    copy_ms = copies[best]["median_ms"]
    copy_rate = 2 * nbytes / (copy_ms * 1e-3)  # a copy moves 2 bytes per byte of the vector
    cases["pbh_hbm_copy"] = dict(copies[best], variant=best, bytes_moved=2 * nbytes,
                                 tb_per_s=round(copy_rate / 1e12, 3))
    del dst

    def edges_of(k, bins):
        return [np.linspace(m["min"], m["max"], bins + 1) for m in (inspection._moment_rows(x)[0] for x in cols[:k])]

    def kernel_case(name, k, bins):
        call = c_call(cols[:k], edges_of(k, bins))
        r = timed(call, a.reps, a.warmup)
        r["pairs"], r["bins"] = call.pairs, bins
        r["bytes_read"] = 16 * n * call.pairs
        rate = r["bytes_read"] / (r["median_ms"] * 1e-3)
        r["tb_per_s"] = round(rate / 1e12, 3)
        r["copy_of_the_same_bytes_ms"] = round(r["bytes_read"] / copy_rate * 1e3, 4)
        r["fraction_of_copy_rate"] = round(rate / copy_rate, 3)
        r["counted_rows_per_pair"] = int(device.to_host(call.counts).sum()) // call.pairs
        cases[name] = r
        print(name, json.dumps({k_: r[k_] for k_ in ("median_ms", "tb_per_s", "fraction_of_copy_rate")}), flush=True)

    kernel_case("pbh_histogram2d_1_pair_64x64", 2, 64)
    kernel_case("pbh_histogram2d_6_pairs_32x32", 4, 32)
    kernel_case("pbh_histogram2d_28_pairs_32x32", 8, 32)
    # how the density's concentration and the LDS footprint move the one-pair figure
    kernel_case("pbh_histogram2d_1_pair_8x8", 2, 8)
    kernel_case("pbh_histogram2d_1_pair_128x128", 2, 128)
    for name, fn in (("histogram2d_64x64", lambda: inspection.histogram2d(ds[0], ds[1], bins=64)),
                     ("pairgrid_4_nodes_32", lambda: inspection.pairgrid(*ds[:4], bins=32)),
                     ("pairgrid_8_nodes_32", lambda: inspection.pairgrid(*ds, bins=32))):
        cases[name] = timed(fn, a.reps, a.warmup)
        print(name, cases[name]["median_ms"], "ms", flush=True)
    assert all(d.__dict__.get("_host") is None for d in ds)
    H, xe, ye = inspection.histogram2d(ds[0], ds[1], bins=64)

    # the existing route, once: both downloads through the pinned ring, then np.histogram2d
    device.synchronize()
    t0 = time.perf_counter()
    x, y = ds[0].samples_, ds[1].samples_
    t1 = time.perf_counter()
    m = min(a.host_rows, n)
    np.histogram2d(x[:m], y[:m], bins=64)
    t2 = time.perf_counter()
    cases["host_route"] = {"download_2_columns_ms": round((t1 - t0) * 1e3, 1), "numpy_histogram2d_rows": m,
                           "numpy_histogram2d_ms_measured": round((t2 - t1) * 1e3, 1),
                           "numpy_histogram2d_ms_scaled_to_n": round((t2 - t1) * 1e3 * n / m, 1),
                           "scaled": m != n, "timer": "wall clock, one run"}
    print("host_route", json.dumps(cases["host_route"]), flush=True)
    if m == n:
        assert np.array_equal(H, np.histogram2d(x, y, bins=64)[0])

    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
