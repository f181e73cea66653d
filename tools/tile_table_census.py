"""How much of the exact cost build could be served from the term table if eligibility were decided per TILE (build container, no GPU).

chi2_sym_kernel tables a (r, theta) shell only where every count of the shell, over all rows of both clouds, is below TL.  A
workgroup needs that only for the 16 moving rows and 64 fixed rows it touches.  This tool builds the frame-1 histograms of
`bench.synth(n)` with the oracle, takes the per-row shell maxima, and reports per shell the fraction of 16 x 64 tiles (natural
row order, as the kernel walks them) whose 80 maxima all stay below TL, with the issue-cycle model of DESIGN.md: a computed
(pair, shell) costs 44 x 4 + 4 x 16 = 240 issue cycles, a tabled one 12 x 4 = 48.

    python tools/tile_table_census.py 50000 20000 > profiles/tile_table_census.txt
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TI, TJ, NSHELL, K = 16, 64, 30, 12
CYC_COMPUTED, CYC_TABLED = 44 * 4 + 4 * 16, 12 * 4


def rowmax_of(oracle, cloud):
    """[n, 30] uint8: per row and shell the largest of the shell's 12 frame-1 counts, saturated at 255 as the kernel's bytes are."""
    c = oracle.get_centroid(cloud, False)
    md = oracle.get_mean_distance(cloud, False)
    x0 = oracle.pca_axis(cloud.T)
    counts, _ = oracle.shape_context_counts(c, md, cloud, "moving", x0=x0)      # frame 1 is frame 1 for either cloud
    return np.minimum(counts[0].reshape(-1, NSHELL, K).max(2), 255).astype(np.uint8)


def tile_ok(rowmax, rows_per_tile, tl):
    """[tiles, 30] bool: every row of the tile below tl in that shell (the ragged last tile holds only its real rows: the kernel's
    clamped indices repeat the last row)."""
    n = rowmax.shape[0]
    nt = (n + rows_per_tile - 1) // rows_per_tile
    pad = np.zeros((nt * rows_per_tile - n, NSHELL), np.uint8)
    return (np.concatenate([rowmax, pad]).reshape(nt, rows_per_tile, NSHELL).max(1) < tl)


def census(n, tl):
    import bench
    import oracle
    oracle.build()
    oracle.set_threads(oracle.host_threads())
    mv, fx, _ = bench.synth(n)
    rm_a, rm_b = rowmax_of(oracle, mv), rowmax_of(oracle, fx)
    ok_a, ok_b = tile_ok(rm_a, TI, tl), tile_ok(rm_b, TJ, tl)
    launch = (rm_a.max(0) < tl) & (rm_b.max(0) < tl)
    # a tile (ti, tj) tables shell g iff ok_a[ti, g] and ok_b[tj, g]: the fraction of tiles is the product of the two fractions
    frac = ok_a.mean(0) * ok_b.mean(0)
    today = np.where(launch, CYC_TABLED, CYC_COMPUTED).sum()
    after = (frac * CYC_TABLED + (1.0 - frac) * CYC_COMPUTED).sum()
    return {"points": n, "table_size": tl, "tile": [TI, TJ], "tiles": [int(ok_a.shape[0]), int(ok_b.shape[0])],
            "shell_max_moving": rm_a.max(0).tolist(), "shell_max_fixed": rm_b.max(0).tolist(),
            "rows_below_tl_moving": (rm_a < tl).mean(0).round(6).tolist(), "rows_below_tl_fixed": (rm_b < tl).mean(0).round(6).tolist(),
            "row_tiles_below_tl": ok_a.mean(0).round(6).tolist(), "column_tiles_below_tl": ok_b.mean(0).round(6).tolist(),
            "tabled_launch_wide": launch.astype(int).tolist(), "tile_fraction_tabled": frac.round(6).tolist(),
            "issue_cycles_per_pair": {"launch_wide": float(today), "per_tile": float(after),
                                      "all_computed": float(NSHELL * CYC_COMPUTED), "all_tabled": float(NSHELL * CYC_TABLED)},
            "predicted_saving_of_launch": float(1.0 - after / today)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("points", type=int, nargs="+")
    ap.add_argument("--tl", type=int, default=94, help="table side (CH_TL)")
    args = ap.parse_args()
    for n in args.points:
        r = census(n, args.tl)
        print(json.dumps(r))
        print("# n = %d, TL = %d: shell: launch-wide | row tiles ok | column tiles ok | tiles tabled" % (n, args.tl))
        for g in range(NSHELL):
            print("#   %2d (max %3d / %3d): %d | %.4f | %.4f | %.4f" % (g, r["shell_max_moving"][g], r["shell_max_fixed"][g],
                                                                     r["tabled_launch_wide"][g], r["row_tiles_below_tl"][g],
                                                                     r["column_tiles_below_tl"][g], r["tile_fraction_tabled"][g]))
        c = r["issue_cycles_per_pair"]
        print("# issue cycles per pair: %.0f launch-wide -> %.1f per tile: %.2f %% of the launch saved" %
              (c["launch_wide"], c["per_tile"], 100.0 * r["predicted_saving_of_launch"]), flush=True)


if __name__ == "__main__":
    main()
