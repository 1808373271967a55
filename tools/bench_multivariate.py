"""Fused multivariate samplers (csrc/pbh_mvar.hip) against the composition of existing entry points
at the same size:

    multivariate_normal  fill_uniform -> pbh_ppf(norm) per column -> pbh_affine_rows
    dirichlet            fill_uniform -> pbh_ppf(gamma) per column -> elementwise sums and divides
    multinomial          fused only (the composition would need d dependent per-row-parameter passes)

Times are device times between two HIP events on the launching stream (torch.cuda.Event on the
current stream), after warm-up calls (which also build and cache the gamma guides), over several
repetitions; the JSON keeps every repetition, the median and the spread.

    python tools/bench_multivariate.py [--n 10000000] [--dims 8 32] [--reps 7] [--warmup 2] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
import probabilit_amd  # noqa: E402,F401
from probabilit_amd import correlation, device, modeling, native  # noqa: E402


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


def ppf_into(name, q, out, **params):
    """native.ppf writing into a row of a preallocated block (no copy afterwards)"""
    from probabilit_amd import _lib

    n = q.shape[0]
    arr, keep = native._params(name, n, params)
    _lib.check(_lib.load().pbh_ppf(_lib.DIST_IDS[name], q.data_ptr(), 1, n, arr, len(arr), out.data_ptr(), None,
                                   device.stream()), "pbh_ppf")


def mvn_case(n, d, reps, warmup):
    rng = np.random.default_rng(d)
    B = rng.normal(size=(d, d))
    cov = B @ B.T / d + 0.1 * np.eye(d)
    mean = rng.normal(size=d)
    A = native.mvn_factor(cov)
    zeros, ones = np.zeros(d), np.ones(d)
    st = {}

    def fill():
        st["u"] = native.fill_uniform(1, n, d, return_device=True)

    def ppf():
        st["z"] = device.empty((d, n))
        for j in range(d):
            ppf_into("norm", st["u"][j], st["z"][j])

    def affine():
        st["x"] = correlation._affine_block(st["z"], zeros, ones, mean, A.T)

    def composed():
        fill(), ppf(), affine()

    out = {"fused": timed(lambda: native.multivariate("multivariate_normal", 1, n, return_device=True, mean=mean,
                                                      cov=cov), reps, warmup),
           "composed": timed(composed, reps, warmup)}
    out["composed_parts"] = {"fill_uniform": timed(fill, reps, 1), "ppf_norm_x_d": timed(ppf, reps, 1),
                             "affine_rows": timed(affine, reps, 1)}
    return out


def dirichlet_case(n, d, reps, warmup):
    alpha = np.random.default_rng(d).choice([0.5, 1.0, 2.5, 7.0], size=d)
    st = {}

    def fill():
        st["u"] = native.fill_uniform(1, n, d, return_device=True)

    def ppf():
        g = device.empty((d, n))
        for j in range(d):
            ppf_into("gamma", st["u"][j], g[j], a=float(alpha[j]))
        st["g"] = list(g)

    def normalise():
        s = st["g"][0]
        for j in range(1, d):
            s = modeling._binary("add", s, st["g"][j], n)
        st["x"] = [modeling._binary("truediv", g, s, n) for g in st["g"]]

    def composed():
        fill(), ppf(), normalise()

    out = {"fused": timed(lambda: native.multivariate("dirichlet", 1, n, return_device=True, alpha=alpha), reps, warmup),
           "composed": timed(composed, reps, warmup)}
    out["composed_parts"] = {"fill_uniform": timed(fill, reps, 1), "ppf_gamma_x_d": timed(ppf, reps, 1),
                             "sum_and_divide": timed(normalise, reps, 1)}
    return out


def multinomial_case(n, d, reps, warmup):
    p = np.random.default_rng(d).dirichlet(np.full(d, 2.0))
    return {"fused": timed(lambda: native.multivariate("multinomial", 1, n, return_device=True, trials=100, p=p), reps,
                           warmup), "trials": 100}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--dims", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    res = {"rows": a.n, "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(device.device()),
           "timer": "HIP events on the launching stream", "cases": {}}
    for d in a.dims:
        for name, case in (("multivariate_normal", mvn_case), ("dirichlet", dirichlet_case),
                           ("multinomial", multinomial_case)):
            r = case(a.n, d, a.reps, a.warmup)
            r["bytes_written"] = 8 * a.n * d
            if "composed" in r:
                r["fused_over_composed"] = round(r["fused"]["median_ms"] / r["composed"]["median_ms"], 4)
            res["cases"][f"{name}_d{d}"] = r
            print(f"{name} d={d}: " + json.dumps({k: (v["median_ms"] if isinstance(v, dict) and "median_ms" in v else v)
                                                  for k, v in r.items() if k != "composed_parts"}), flush=True)
            device.synchronize()
            torch.cuda.empty_cache()
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
