#!/usr/bin/env python3
"""Pruning power and speed of the Hellinger candidate lists (K.hellinger_topk; csrc/pm_hellinger.hip) on the bench clouds, measured
with the product's own kernels — the two kill criteria of VERDICT.md "Next round" item 1:
  (i)  share of rows whose MATCHED column (the exact mode's assignment) lies inside the bound's top-k of the row;
  (ii) share of a row's columns whose bound lies below the row's 16th-smallest EXACT cost (what a per-row threshold cannot prune).
Per pairing (U11, U12, U13, U14), for k = 16, 32, 64, plus the largest |L~ - L_float64| seen on sampled rows.
Usage: python tools/hellinger_power.py [N=20000] [--rows R] [--speed] [--only-kernel] [--list] [--select] [--nearest]
  --rows R       criteria on R evenly spaced rows instead of all (50 000 nuclei: the exact matrix of R rows at a time)
  --speed        also time hellinger_topk(k=16, four frames) against chi2_filter4(float32) + pm_lsap_row_select_f32(k=16) on the
                 four matrices: alternating, seven repetitions each after a warm-up, HIP events around work that ends in a synchronise
  --only-kernel  descriptors + one warm-up + one hellinger_topk call, nothing else (the subject of a rocprofv3 --kernel-trace run)
  --list         the threshold listing (K.hellinger_list) and nothing else: its speed against hellinger_topk(k=16) at about 16
                 entries per row (u = the row's 16th bound, v = 0, tau = 0; alternating, seven repetitions each), and the LIST SIZE
                 of a matrix-free pricing round: entries listed per row under the final duals of the exact mode's device solve
  --select       the priced selection (K.hellinger_select) and nothing else: its speed against hellinger_topk(k=16) at k = 16 and
                 k = 8, with v = 0 and with v = the bound's column minima (alternating, seven repetitions each after a warm-up);
                 the same four legs with precision='bf16x3' (csrc/pm_hellinger_bf16.hip) alternate with them in the same process,
                 followed by the ratio at k = 16 against three times the larger min-max spread, and the largest
                 |bound - L_float64| of the bf16x3 lists over all rows
  --nearest      the exact rescoring (K.chi2_select_exact) and nothing else: from the same hellinger_select(k=32) lists, F = 4, k = 8,
                 the one-launch kernel against the same answer by the chain a resident-matrix selector runs (mask, gathers,
                 K.chi2_entries per pairing, scatter, price gather, argsort, gathers), with v = 0 and v = the bound's column minima
                 (alternating, seven repetitions each after a warm-up), and the share of units with proven == k — also from
                 bf16x3 candidate lists under their delta (K.chi2_nearest(precision='bf16x3'))
(--list also reports the list size at the bf16x3 delta: the same listing kernel under tau formed with cost_delta = delta_bf16x3.)
Prints to stdout; writes nothing."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", nargs="?", type=int, default=20000)
    ap.add_argument("--rows", type=int, default=0)
    ap.add_argument("--speed", action="store_true")
    ap.add_argument("--only-kernel", action="store_true")
    ap.add_argument("--list", action="store_true")
    ap.add_argument("--select", action="store_true")
    ap.add_argument("--nearest", action="store_true")
    args = ap.parse_args()
    import torch
    import bench
    from platymatch_amd import _kernels as K, _native as nat, lsap as L, pipeline as P
    from platymatch_amd.estimate_transform import perform_icp as pi
    pi.VERBOSE = False
    n = args.n
    mv, fx, _ = bench.synth(n)
    be = P.GpuBackend()
    sc_m, sc_f, _ = P.build_descriptors(be, be.cloud(mv), be.cloud(fx))
    a = sc_m[0].contiguous()
    delta = K.hellinger_delta()
    print("hellinger_power: %d x %d nuclei (bench.synth), delta = %.3g" % (n, n, delta))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    if args.only_kernel:
        for _ in range(2):
            ms, _ = timed(lambda: K.hellinger_topk(a, sc_f, k=16))
        print("hellinger_topk(k=16, 4 frames): %.2f ms = %.1f TFLOP/s of 2*360*F*N*M" % (ms, 2 * 360 * 4 * n * n / ms / 1e9))
        return

    if args.list:
        list_leg(torch, K, L, a, sc_m, sc_f, n, delta, timed, K.hellinger_delta("bf16x3"))
        return

    if args.select:
        select_leg(torch, K, a, sc_f, n, timed)
        return

    if args.nearest:
        nearest_leg(torch, K, a, sc_f, n, timed)
        return

    if args.speed:
        lib = nat.load()
        U = torch.empty((4, n, n), dtype=torch.float32, device=a.device)
        cols = torch.empty((n, 16), dtype=torch.int32, device=a.device)
        costs = torch.empty((n, 16), dtype=torch.float64, device=a.device)
        flag = torch.empty(1, dtype=torch.int32, device=a.device)

        def old():
            K.chi2_filter4(a, sc_f[0].contiguous(), out=U)
            for t in range(4):
                nat.check(lib.pm_lsap_row_select_f32(nat.ptr(U[t]), n, n, n, None, 16, nat.ptr(cols), nat.ptr(costs), nat.ptr(flag), nat.stream_ptr(U)))

        def new():
            K.hellinger_topk(a, sc_f, k=16)
        old(), new()
        t_old, t_new = [], []
        for _ in range(7):
            t_old.append(timed(old)[0])
            t_new.append(timed(new)[0])
        for name, t in (("chi2_filter4(float32) + 4 x row_select_f32(k=16)", t_old), ("hellinger_topk(k=16, 4 frames)", t_new)):
            print("speed  %-50s median %8.2f ms  min %8.2f  max %8.2f  (7 repetitions, alternating)" % (name, np.median(t), min(t), max(t)))
        print("speed  hellinger_topk: %.1f TFLOP/s of the algorithmic 2*360*F*N*M flop" % (2 * 360 * 4 * n * n / np.median(t_new) / 1e9))
        del U

    details = {}
    P.estimate_transform(mv, fx, cost_mode="exact", seed=0, icp_iterations=1, ransac_trials=100, details=details)
    rows = np.arange(n) if not args.rows else np.unique(np.linspace(0, n - 1, args.rows).astype(np.int64))
    sym = K.chi2_symmetric(sc_m, sc_f)
    cols_t, bound_t = K.hellinger_topk(a, sc_f, k=64)
    cols, bound = cols_t.cpu().numpy(), bound_t.cpu().numpy()
    worst = 0.0
    step = 2048
    for t in range(4):
        r_h, c_h = details["lsa"][L.PAIRINGS[t][0]]
        match = np.full(n, -1, np.int64)
        match[np.asarray(r_h)] = np.asarray(c_h)
        below, total = 0, 0
        for r0 in range(0, len(rows), step):
            rr = torch.as_tensor(rows[r0:r0 + step], device=a.device)
            sub = sc_m[:, rr].contiguous()
            C = K.chi2_cost_pair(sub, sc_f, t, sym)[0]                        # the exact natural-order matrix of these rows
            c16 = torch.kthvalue(C, 16, dim=1).values
            ra, rb = torch.sqrt(sub[0]), torch.sqrt(sc_f[t])
            Lref = 0.5 * (sub[0].sum(1)[:, None] + sc_f[t].sum(1)[None, :]) - ra @ rb.T          # float64 on the device: the yardstick only
            below += int((Lref < c16[:, None]).sum())
            total += C.numel()
            assert bool((Lref <= C + 1e-12).all()), "the bound exceeds the exact cost"
            got = torch.gather(Lref, 1, cols_t[t, rr].long().clamp(min=0))
            worst = max(worst, float((got - bound_t[t, rr]).abs().max()))
        line = "pairing %d (U1%d): (ii) columns with bound below the row's 16th exact cost: %.2f %%;  (i) matched column listed:" % (t, t + 1, 100.0 * below / total)
        for k in (16, 32, 64):
            hit = (cols[t, rows, :k] == match[rows, None]).any(1)
            line += "  k=%d %.2f %%" % (k, 100.0 * hit[match[rows] >= 0].mean())
        print(line)
    print("largest |bound - L_float64| on listed entries: %.3g (delta %.3g)" % (worst, delta))


def list_leg(torch, K, L, a, sc_m, sc_f, n, delta, timed, delta_bf):
    import types
    flop = 2 * 360 * 4 * n * n
    kth = K.hellinger_topk(a, sc_f, k=16)[1][:, :, 15].contiguous()
    zero, info = torch.zeros((4, n), dtype=torch.float64, device=a.device), {}

    def new():
        return K.hellinger_list(a, sc_f, kth, zero, 0.0, info=info)

    def old():
        out = K.hellinger_topk(a, sc_f, k=16)
        torch.cuda.synchronize()                  # (hellinger_list reads its counts back: both legs end in a synchronise)
        return out
    old(), new()
    t_old, t_new = [], []
    for _ in range(7):
        t_old.append(timed(old)[0])
        t_new.append(timed(new)[0])
    print("list   entries per row at u = 16th bound, v = 0, tau = 0: %s" % ", ".join("%.2f" % (c / n) for c in info["count"]))
    for name, t in (("hellinger_topk(k=16, 4 frames)", t_old), ("hellinger_list(4 frames), sort by (row, column) included", t_new)):
        print("speed  %-58s median %8.2f ms  min %8.2f  max %8.2f  %6.1f TFLOP/s  (7 repetitions, alternating)"
              % (name, np.median(t), min(t), max(t), flop / np.median(t) / 1e9))
    sym = K.chi2_symmetric(sc_m, sc_f)
    for t in range(4):
        U = K.chi2_cost_pair(sc_m, sc_f, t, sym)[0]
        sol = L.solve_core(L.DeviceMatrix(U), {})
        del U
        if sol is None:
            print("pairing %d: the device solve gave no duals" % t)
            continue
        u, v, col4row = (np.asarray(x) for x in sol)
        tau = L.FilteredMatrix._tau(types.SimpleNamespace(cost_delta=delta), u, v)
        dev = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x), dtype=dt).to(a.device)
        got = K.hellinger_list(a, sc_f[t].contiguous(), dev(u, torch.float64), dev(v, torch.float64), tau,
                               skip=dev(col4row, torch.int32), cap=256 * n, info=info)[0]
        per_row = torch.bincount(got[0].long(), minlength=n) if got is not None else None
        print("pairing %d (U1%d): tau = %.3g; listed under the final duals: %d entries = %.2f per row (max %s); exceeds 64 * M: %s"
              % (t, t + 1, tau, info["count"][0], info["count"][0] / n, "?" if per_row is None else int(per_row.max()),
                 "YES" if info["count"][0] > 64 * n else "no"))
        tau = L.FilteredMatrix._tau(types.SimpleNamespace(cost_delta=delta_bf), u, v)
        K.hellinger_list(a, sc_f[t].contiguous(), dev(u, torch.float64), dev(v, torch.float64), tau, skip=dev(col4row, torch.int32),
                         cap=256 * n, info=info)
        print("pairing %d (U1%d): at the bf16x3 delta %.3g, tau = %.3g: %d entries = %.2f per row; exceeds 64 * M: %s"
              % (t, t + 1, delta_bf, tau, info["count"][0], info["count"][0] / n, "YES" if info["count"][0] > 64 * n else "no"))


def select_leg(torch, K, a, sc_f, n, timed):
    flop = 2 * 360 * 4 * n * n
    zero = torch.zeros((4, n), dtype=torch.float64, device=a.device)
    # the bound's column minima: the top-1 of the transposed problem, frame by frame (the bound is symmetric in its arguments)
    vmin = torch.stack([K.hellinger_topk(sc_f[f].contiguous(), a, k=1)[1][0, :, 0] for f in range(4)]).contiguous()

    def leg(fn):
        def run():
            out = fn()
            torch.cuda.synchronize()
            return out
        return run
    legs = [("hellinger_topk(k=16, 4 frames)", leg(lambda: K.hellinger_topk(a, sc_f, k=16)))]
    for k in (16, 8):
        for name, v in (("v = 0", zero), ("v = column minima", vmin)):
            legs.append(("hellinger_select(k=%d, %s)" % (k, name), leg(lambda k=k, v=v: K.hellinger_select(a, sc_f, v=v, k=k))))
            legs.append(("hellinger_select(k=%d, %s, bf16x3)" % (k, name),
                         leg(lambda k=k, v=v: K.hellinger_select(a, sc_f, v=v, k=k, precision="bf16x3"))))
    outs = [run() for _, run in legs]                     # warm-up; and the unpriced lists are the top-k kernel's, bit for bit
    same = torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1].view(torch.int64), outs[1][1].view(torch.int64))
    print("select (k=16, v = 0) against hellinger_topk(k=16): columns and bound bits %s" % ("identical" if same else "DIFFER"))
    moved = (outs[3][0] != outs[0][0]).any(dim=2).float().mean().item()
    print("select rows whose list changes under v = column minima: %.1f %%" % (100.0 * moved))
    times = [[] for _ in legs]
    for _ in range(7):
        for t, (_, run) in zip(times, legs):
            t.append(timed(run)[0])
    for (name, _), t in zip(legs, times):
        print("speed  %-46s median %8.2f ms  min %8.2f  max %8.2f  %6.1f TFLOP/s  (7 repetitions, alternating)"
              % (name, np.median(t), min(t), max(t), flop / np.median(t) / 1e9))
    t32, tbf = times[1], times[2]                        # k = 16, v = 0: float32 and bf16x3
    spread = max(max(t32) - min(t32), max(tbf) - min(tbf))
    print("select k = 16, v = 0: float32 %.2f ms / bf16x3 %.2f ms = %.2f x; difference %.2f ms against 3 x the larger min-max spread = %.2f ms"
          % (np.median(t32), np.median(tbf), np.median(t32) / np.median(tbf), np.median(t32) - np.median(tbf), 3 * spread))
    delta_bf, worst, same = K.hellinger_delta("bf16x3"), 0.0, 0.0
    cols_b, bound_b = outs[2]
    ra, rb, ha = torch.sqrt(a), torch.sqrt(sc_f), 0.5 * a.sum(1)
    for f in range(4):
        hb = 0.5 * sc_f[f].sum(1)
        for r0 in range(0, n, 2048):
            Lref = (ha[r0:r0 + 2048, None] + hb[None, :]) - ra[r0:r0 + 2048] @ rb[f].T      # float64 on the device: the yardstick only
            got = torch.gather(Lref, 1, cols_b[f, r0:r0 + 2048].long().clamp(min=0))
            worst = max(worst, float((got - bound_b[f, r0:r0 + 2048]).abs().max()))
    same = (torch.sort(cols_b, dim=2).values == torch.sort(outs[1][0], dim=2).values).all(dim=2).float().mean().item()
    print("select bf16x3 (k=16, v = 0): largest |bound - L_float64| over all %d x 4 x 16 listed entries: %.3g (delta %.3g); rows "
          "whose column SET equals the float32 list's: %.2f %%" % (n, worst, delta_bf, 100.0 * same))


def nearest_leg(torch, K, a, sc_f, n, timed, candidates=32, k=8):
    zero = torch.zeros((4, n), dtype=torch.float64, device=a.device)
    vmin = torch.stack([K.hellinger_topk(sc_f[f].contiguous(), a, k=1)[1][0, :, 0] for f in range(4)]).contiguous()
    b1 = sc_f[0].contiguous()
    rows_all = torch.arange(n, dtype=torch.int32, device=a.device)[:, None].expand(n, candidates)

    def chain(lists, v):
        """lsap.FilteredMatrix._row_select_t's steps around K.chi2_entries, pairing by pairing, cut to k"""
        out_c, out_x = [], []
        for f in range(4):
            cols = lists[0][f]
            valid = cols >= 0
            exact = K.chi2_entries(a, b1, f, rows_all[valid].contiguous(), cols[valid].contiguous(), trusted=True)[0]
            costs = torch.full(cols.shape, float("inf"), dtype=torch.float64, device=cols.device)
            costs[valid] = exact
            red = costs - v[f][cols.clamp(min=0).long()]
            order = torch.argsort(torch.where(valid, red, torch.full_like(red, float("inf"))), dim=1, stable=True)[:, :k]
            out_c.append(torch.gather(cols, 1, order)), out_x.append(torch.gather(costs, 1, order))
        torch.cuda.synchronize()
        return torch.stack(out_c), torch.stack(out_x)

    def kernel(lists, v):
        out = K.chi2_select_exact(a, sc_f, lists[0], lists[1], v=v, k=k)
        torch.cuda.synchronize()
        return out
    legs = []
    for name, v in (("v = 0", zero), ("v = column minima", vmin)):
        lists = K.hellinger_select(a, sc_f, v=v, k=candidates)
        legs.append(("chain around chi2_entries (%s)" % name, lambda lists=lists, v=v: chain(lists, v)))
        legs.append(("chi2_select_exact (%s)" % name, lambda lists=lists, v=v: kernel(lists, v)))
    outs = [run() for _, run in legs]                     # warm-up; and both routes give the same answer
    for i in (0, 2):
        same = torch.equal(outs[i][0], outs[i + 1][0]) and torch.equal(outs[i][1].view(torch.int64), outs[i + 1][1].view(torch.int64))
        full = (outs[i + 1][2] == k).float().mean().item()
        print("nearest %-20s columns and cost bits of the two routes %s; units with proven == k: %.2f %%, mean proven %.2f of %d"
              % (legs[i + 1][0][18:], "identical" if same else "DIFFER", 100.0 * full, outs[i + 1][2].float().mean().item(), k))
    for name, v in (("v = 0", zero), ("v = column minima", vmin)):
        for prec in ("f32", "bf16x3"):
            pr = K.chi2_nearest(a, sc_f, v=v, k=k, candidates=candidates, precision=prec)[2]
            print("nearest %-20s candidates from %-6s (delta %.3g): units with proven == k: %.2f %%, mean proven %.2f of %d"
                  % (name, prec, K.hellinger_delta(prec), 100.0 * (pr == k).float().mean().item(), pr.float().mean().item(), k))
    times = [[] for _ in legs]
    for _ in range(7):
        for t, (_, run) in zip(times, legs):
            t.append(timed(run)[0])
    for (name, _), t in zip(legs, times):
        print("speed  %-46s median %8.2f ms  min %8.2f  max %8.2f  (7 repetitions, alternating; %d x %d, F = 4, candidates = %d, k = %d)"
              % (name, np.median(t), min(t), max(t), n, n, candidates, k))


if __name__ == "__main__":
    main()
