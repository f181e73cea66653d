"""What a shell costs the exact cost build when it is served from the term table, by the RANGE of its counts, against computing it.

Synthetic descriptors (integer counts over one common total, N x N, every shell alike) through K.chi2_frame1_tile_report:
    computed      every row holds one count of 94 per shell: no tile tables anything
    tabled 0..R   counts uniform in 0..R (R = 8, 31, 63, 93): every tile tables all thirty shells
A wave reads ONE table row per (moving row, bin), its 64 lanes at the columns' counts: equal counts broadcast, counts 32 apart
share LDS banks.  The wider the range, the more distinct addresses and bank conflicts per read.

    python tools/tile_table_shell_cost.py [N]        -> one line per case: build ms (HIP events, median of 5), ms per shell"""
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
    total = 4096.0
    tiles = ((n + 15) // 16) * ((n + 63) // 64)
    base = None
    for name, hi, spoil in (("computed", 31, True), ("tabled 0..8", 8, False), ("tabled 0..31", 31, False), ("tabled 0..63", 63, False),
                            ("tabled 0..93", 93, False), ("tabled 62..93", -93, False)):
        lo = 62 if hi < 0 else 0
        ca, cb = (rng.integers(lo, abs(hi) + 1, (n, 360)) for _ in range(2))
        ca[:, 0], cb[:, 0] = 1, 1
        if spoil:
            ca[:, 5::12] = 94
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
        frac = float(tabled.sum().item()) / (30.0 * tiles)
        med = float(np.median(ms[1:]))
        base = med if base is None else base
        print("%-14s N = %d: build %8.2f ms, %6.3f ms per shell, %.3f of computed; (tile, shell) pairs tabled: %.3f"
              % (name, n, med, med / 30.0, med / base, frac), flush=True)


if __name__ == "__main__":
    main()
