"""The exact cost build alone at N x N nuclei of the bench clouds: HIP-event time of K.chi2_cost8_frame1 (counts pre-pass + the
half-cost kernel) on the product's own descriptors, and which tiles took which shell from the term table.

    python tools/chi2_build_timing.py 20000 [--reps 10] [--dump FILE.npy]

Prints one JSON line.  --dump writes a seeded sample of the eight matrices' bits (for comparing two builds of the library)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("points", type=int)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--dump")
    args = ap.parse_args()
    import torch
    import bench
    from platymatch_amd import _kernels as K, _native as nat, pipeline as P
    nat.load()
    n = args.points
    mv, fx, _ = bench.synth(n)
    be = P.GpuBackend()
    sc_m, sc_f, _ = P.build_descriptors(be, be.cloud(mv), be.cloud(fx))
    assert K.chi2_symmetric(sc_m, sc_f)
    U = torch.empty((8, n, n), dtype=torch.float64, device=sc_m.device)
    info = {}
    K.chi2_cost8_frame1(sc_m[0], sc_f[0], out=U, info=info)             # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        K.chi2_cost8_frame1(sc_m[0], sc_f[0], out=U)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    rec = {"points": n, "reps": args.reps, "build_ms": {"min": min(ms), "median": float(np.median(ms)), "max": max(ms)},
           "tabled_launch_wide": info.get("tabled_shells"), "seedable_launch_wide": info.get("seedable_shells"),
           "seeded_pairings_env": os.environ.get("PM_CHI2_SEED")}
    if hasattr(K, "chi2_frame1_tile_report"):
        del U
        _, tabled, tiles = K.chi2_frame1_tile_report(sc_m[0], sc_f[0])
        rec["tiles"] = tiles
        rec["tile_fraction_tabled"] = [round(float(x) / tiles, 6) for x in tabled.cpu().numpy()]
        U = _
    if args.dump:
        idx = torch.as_tensor(np.random.default_rng(0).integers(0, n * n, 1 << 20), device=U.device)
        np.save(args.dump, U.reshape(8, -1)[:, idx].contiguous().view(torch.int64).cpu().numpy())
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
