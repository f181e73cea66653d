"""What a shell costs the exact cost build when its divisions are seeded from the count-sum table, against div_pos and against
the term table: the sibling of tile_table_shell_cost.py for csrc/pm_chi2.hip's NSP path.

Synthetic descriptors (integer counts over one common total of 20 000, N x N, every shell alike) through
K.chi2_frame1_tile_report, with PM_CHI2_SEED = 0 (every term by div_pos), 4 (all four pairings of a row seeded) and 2 (two of
them), for counts in 100..400 (few distinct sums per gather) and 100..4000 (64 scattered addresses per gather); and one tabled
case (counts 0..93) for scale.

    python tools/seeded_shell_cost.py [N]        -> one line per case: build ms (HIP events, median of 5), ms per shell"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
    import torch
    from platymatch_amd import _kernels as K, _native as nat
    nat.load()
    rng = np.random.default_rng(1)
    total = 20000.0
    base = None
    for name, lo, hi, mode in (("computed 100..4000", 100, 4000, "0"), ("seeded4 100..400", 100, 400, "4"), ("seeded4 100..4000", 100, 4000, "4"),
                               ("seeded2 100..400", 100, 400, "2"), ("seeded2 100..4000", 100, 4000, "2"), ("tabled 0..93", 0, 93, "0")):
        os.environ["PM_CHI2_SEED"] = mode             # (the library reads it per launch)
        ca, cb = (rng.integers(lo, hi + 1, (n, 360)) for _ in range(2))
        ca[:, 0], cb[:, 0] = 1, 1
        a, b = nat.to_dev(ca / total), nat.to_dev(cb / total)
        ms = []
        for rep in range(6):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out, tabled, t = K.chi2_frame1_tile_report(a, b)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
            del out
        med = float(np.median(ms[1:]))
        base = med if base is None else base
        print("%-20s N = %d: build %8.2f ms, %6.3f ms per shell, %.3f of computed; shells tabled in every tile: %d"
              % (name, n, med, med / 30.0, med / base, int((tabled == t).sum().item())), flush=True)


if __name__ == "__main__":
    main()
