"""What does a wavefront range of k_spmv_range cost?  The fit behind csrc/csr5_range_cut.h (A, B, C and the slot table).

Needs the experiment build of the library (wall-clock stamps per range, the cut pass's per-tile counts and the cut table as debug exports):
    make -C benchmark_spmv_using_csr5_amd/csrc stamps STAMPS_DEFS="-DCSR5_RANGE_COST_B=0 -DCSR5_RANGE_COST_C=0"     # equal-count cuts
    CSR5HIP_LIB=benchmark_spmv_using_csr5_amd/libcsr5hip_stamps.so python scripts/experiments/range_cost_fit.py --out DIR
(without STAMPS_DEFS the build cuts by the header's constants: the same script then shows what the cuts achieved.)

R-MAT 24 at the bench's parameters, library defaults: least squares of the duration of the 4 096 ranges (one SpMV, medians over --reps
SpMVs) on tiles, cold lanes, row starts and the wavefront slot; the coefficients are then held against R-MAT 22 WITHOUT refitting.  Also the
figures profiles/r05_probes.txt section 2 gave: per slab max / mean, per workgroup max-of-8 / mean, the spread of the range ends.
Raw per-range data goes to DIR/range_cost_rmat<scale>.npz, the report to stdout and DIR/range_cost_fit.txt."""
import argparse
import ctypes as C
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

RANGES, WAVES = 256, 8
LINES = []


def say(*words):
    line = " ".join(str(w) for w in words)
    LINES.append(line)
    print(line, flush=True)


def measure(scale, reps):
    import torch

    import bench as B
    from benchmark_spmv_using_csr5_amd import _capi

    dev = torch.device("cuda", 0)
    a = types.SimpleNamespace(values="int", sigma="-1", mode="fused", x_window="auto", xcd_remap=1, lds_y="auto", stream_nt="auto", slabs="auto",
                              slab_shift=None, slab_hot="auto", x_snapshot=0, zero_empty=0, seed=1, full=False)
    mat, label = B.make_shard(f"rmat{scale}", 0, 1, a.seed, np.float64, dev, 1.0, True, None)
    prob = B.Problem(mat, label, "f64", a, dev, a.seed + 13)
    S = prob.info.column_slabs
    assert prob.info.slab_hot == 1 and 0 < S <= 64, (prob.info.slab_hot, S)
    lib = _capi.load()
    for name, t in (("csr5hip_debug_range_stamps", C.c_void_p), ("csr5hip_debug_tile_stats", C.c_void_p), ("csr5hip_debug_cut_table", C.c_void_p)):
        getattr(lib, name).argtypes = [t, C.c_int]
    table = np.zeros(S * (RANGES + 1), dtype=np.int32)
    assert lib.csr5hip_debug_cut_table(table.ctypes.data, table.size) == 0
    table = table.reshape(S, RANGES + 1)
    tiles_all = int(table.max())
    stats = np.zeros(tiles_all, dtype=np.uint32)
    assert lib.csr5hip_debug_tile_stats(stats.ctypes.data, stats.size) == 0
    for _ in range(3):
        prob.A.spmv(1.0, prob.yd)
    torch.cuda.synchronize()
    starts_us, ends_us = [], []
    for _ in range(reps):
        prob.A.spmv(1.0, prob.yd)
        torch.cuda.synchronize()
        buf = np.zeros(2 * S * RANGES, dtype=np.uint64)
        assert lib.csr5hip_debug_range_stamps(buf.ctypes.data, buf.size) == 0
        t0, t1 = buf[0::2].astype(np.int64).reshape(S, RANGES), buf[1::2].astype(np.int64).reshape(S, RANGES)
        base = t0[t0 > 0].min()
        starts_us.append((t0 - base) / 100.0)
        ends_us.append((t1 - base) / 100.0)
    cold_t, starts_t = (stats & 0xFFFF).astype(np.int64), (stats >> 16).astype(np.int64)
    cc, cs = np.concatenate([[0], np.cumsum(cold_t)]), np.concatenate([[0], np.cumsum(starts_t)])
    d = dict(scale=scale, S=S, table=table, tiles=np.diff(table, axis=1), cold=cc[table[:, 1:]] - cc[table[:, :-1]],
             starts=cs[table[:, 1:]] - cs[table[:, :-1]], start_us=np.array(starts_us), end_us=np.array(ends_us), nnz=prob.nnz)
    prob.A.destroy()
    prob.A.close()
    del prob, mat
    torch.cuda.empty_cache()
    return d


def describe(d):
    S = d["S"]
    dur = np.median(d["end_us"] - d["start_us"], axis=0)
    end = np.median(d["end_us"], axis=0)
    say(f"R-MAT {d['scale']}: {S} slabs, kernel span {end.max():.1f} us; tiles per range {d['tiles'].min()}..{d['tiles'].max()}, "
        f"cold lanes per range / slab mean {(d['cold'] / d['cold'].mean(axis=1, keepdims=True)).min():.3f}.."
        f"{(d['cold'] / d['cold'].mean(axis=1, keepdims=True)).max():.3f}, row starts {(d['starts'] / d['starts'].mean(axis=1, keepdims=True)).min():.3f}.."
        f"{(d['starts'] / d['starts'].mean(axis=1, keepdims=True)).max():.3f}")
    wg = dur.reshape(S, 32, WAVES)
    say(f"  per slab max/mean of the range time: {np.round(dur.max(axis=1) / dur.mean(axis=1), 3).tolist()}")
    say(f"  per workgroup max-of-8 over mean-of-8: mean {np.mean(wg.max(axis=2) / wg.mean(axis=2)):.4f}, worst {np.max(wg.max(axis=2) / wg.mean(axis=2)):.4f}")
    order = np.argsort(np.median(d["start_us"], axis=0).min(axis=1))
    last = order[S // 2:] if S > 8 else order
    say(f"  ends of the last round's ranges: {end[last].min():.1f} .. {end[last].max():.1f} us (spread {end[last].max() - end[last].min():.1f}); "
        f"per slab spread of the ends, mean {np.mean(end.max(axis=1) - end.min(axis=1)):.1f} us")
    say(f"  run to run: median over ranges of (max - min) / median of the duration = "
        f"{np.median(np.ptp(d['end_us'] - d['start_us'], axis=0) / dur):.4f}")
    return dur


def design(d, with_slot, with_work, with_slab):
    """columns: the work terms, the slots 1 .. 7 (slot 0 is the base), then one level per slab or one for all"""
    S = d["S"]
    cols, names = [], []
    if with_work:
        cols += [d["tiles"].ravel().astype(float), d["cold"].ravel().astype(float), d["starts"].ravel().astype(float)]
        names += ["tile", "cold", "start"]
    if with_slot:
        slot = np.tile(np.arange(RANGES) % WAVES, S)
        for j in range(1, WAVES):
            cols.append((slot == j).astype(float))
            names.append(f"slot{j}")
    if with_slab:
        slab = np.repeat(np.arange(S), RANGES)
        for k in range(S):
            cols.append((slab == k).astype(float))
            names.append(f"slab{k}")
    else:
        cols.append(np.ones(S * RANGES))
        names.append("level")
    return np.stack(cols, axis=1), names


def r2(y, pred):
    return 1.0 - np.sum((y - pred) ** 2) / np.sum((y - y.mean()) ** 2)


def fit(d, dur):
    y = dur.ravel()
    out = {}
    for tag, (sl, wk, sb) in (("slot alone", (1, 0, 0)), ("tiles + cold + starts", (0, 1, 0)), ("tiles + cold + starts + slot", (1, 1, 0)),
                              ("slab alone", (0, 0, 1)), ("slot + slab", (1, 0, 1)), ("tiles + cold + starts + slab", (0, 1, 1)),
                              ("tiles + cold + starts + slot + slab", (1, 1, 1))):
        X, names = design(d, sl, wk, sb)
        beta, *_ = np.linalg.lstsq(X, y, rcond=None)
        out[tag] = (names, beta, r2(y, X @ beta))
        say(f"  R^2 {tag:38s} {out[tag][2]:.4f}")
    return out


def levels(d, dur):
    """The same regression with the levels taken out one by one: (slab, slot) means; (slab, workgroup) means and slot means -- what a
    wavefront pays relative to the other seven of its workgroup --; and the workgroups' means alone (slab means taken out)."""
    S = d["S"]

    def take(x, level):
        x = x.reshape(S, 32, WAVES).astype(float).copy()
        if level == "within slab and slot":
            x -= x.mean(axis=1, keepdims=True)
        elif level == "within workgroup":
            x -= x.mean(axis=2, keepdims=True)
            x -= x.mean(axis=1, keepdims=True)
        else:
            x = x.mean(axis=2)
            x -= x.mean(axis=1, keepdims=True)
        return x.ravel()

    out = {}
    for level in ("within slab and slot", "within workgroup", "between workgroups"):
        y = take(dur, level)
        X = np.stack([take(d["tiles"], level), take(d["cold"], level), take(d["starts"], level)], axis=1)
        beta, *_ = np.linalg.lstsq(X, y, rcond=None)
        out[level] = beta
        say(f"  {level:22s}: sd {y.std():6.2f} us; us per tile {beta[0]:8.4f}, per cold lane {beta[1]:9.6f}, per row start {beta[2]:9.6f}; "
            f"R^2 {1 - np.sum((y - X @ beta) ** 2) / np.sum(y ** 2):.4f}")
    out["take"] = take
    return out


def slab_level(d, dur):
    t, c, s = d["tiles"].sum(axis=1), d["cold"].sum(axis=1), d["starts"].sum(axis=1)
    per_tile = dur.sum(axis=1) / t
    say(f"  per slab: us per tile {np.round(per_tile, 3).tolist()}")
    say(f"            cold lanes per tile {np.round(c / t, 1).tolist()}; correlation of the two {np.corrcoef(per_tile, c / t)[0, 1]:.3f}, "
        f"slope {np.polyfit(c / t, per_tile, 1)[0]:.5f} us per cold lane")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True, help="directory for the raw per-range data and the report")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--scales", default="24,22")
    ap.add_argument("--from-npz", action="store_true", help="refit from the raw data of an earlier run in --out (no GPU)")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    scales = [int(s) for s in args.scales.split(",")]
    data = {}
    for sc in scales:
        path = os.path.join(args.out, f"range_cost_rmat{sc}.npz")
        if args.from_npz:
            data[sc] = dict(np.load(path))
            data[sc] = {k: (v.item() if v.ndim == 0 else v) for k, v in data[sc].items()}
        else:
            data[sc] = measure(sc, args.reps)
            np.savez_compressed(path, **data[sc])
    fit_scale = scales[0]
    dur = {sc: describe(data[sc]) for sc in scales}
    say(f"least squares on R-MAT {fit_scale} ({dur[fit_scale].size} ranges):")
    fits = fit(data[fit_scale], dur[fit_scale])
    lv = {}
    for sc in scales:
        say(f"R-MAT {sc}, the work terms level by level (mean us per tile {np.mean(dur[sc] / np.maximum(data[sc]['tiles'], 1)):.3f}, cold lanes per tile "
            f"{data[sc]['cold'].sum() / data[sc]['tiles'].sum():.1f}, row starts per tile {data[sc]['starts'].sum() / data[sc]['tiles'].sum():.1f}):")
        lv[sc] = levels(data[sc], dur[sc])
        slab_level(data[sc], dur[sc])
    for sc in scales[1:]:
        take, beta = lv[sc]["take"], lv[fit_scale]["within workgroup"]
        y = take(dur[sc], "within workgroup")
        X = np.stack([take(data[sc][k], "within workgroup") for k in ("tiles", "cold", "starts")], axis=1)
        say(f"R-MAT {sc} within workgroup with R-MAT {fit_scale}'s coefficients, nothing refitted: R^2 {1 - np.sum((y - X @ beta) ** 2) / np.sum(y ** 2):.4f}")
    for sc in scales:  # what levelling the explained part inside every workgroup would buy
        take, beta, S = lv[sc]["take"], lv[fit_scale]["within workgroup"], data[sc]["S"]
        X = np.stack([take(data[sc][k], "within workgroup") for k in ("tiles", "cold", "starts")], axis=1)
        full = dur[sc].reshape(S, 32, WAVES)
        left = (take(dur[sc], "within workgroup") - X @ beta).reshape(S, 32, WAVES)
        slot = (full - full.mean(axis=2, keepdims=True)).mean(axis=1, keepdims=True)
        say(f"R-MAT {sc}: workgroup max-of-8 / mean-of-8 {np.mean(full.max(axis=2) / full.mean(axis=2)):.4f} now; with the explained part levelled "
            f"{np.mean((full.mean(axis=2, keepdims=True) + slot + left).max(axis=2) / full.mean(axis=2)):.4f}; with the slots levelled too "
            f"{np.mean((full.mean(axis=2, keepdims=True) + left).max(axis=2) / full.mean(axis=2)):.4f}")
    for tag in ("tiles + cold + starts + slot", "tiles + cold + starts + slot + slab"):
        names, beta, _ = fits[tag]
        co = dict(zip(names, beta))
        say(f"  [{tag}] us per tile {co['tile']:.4f}, per cold lane {co['cold']:.6f}, per row start {co['start']:.6f}; "
            f"A : B : C = 1000 : {1000 * co['cold'] / co['tile']:.2f} : {1000 * co['start'] / co['tile']:.2f}; "
            f"slot terms (us, slot 0 = 0): {[round(float(co[f'slot{j}']), 2) for j in range(1, WAVES)]}")
    # the slot as a FACTOR on the modelled work (what the cut table's per-slot shares mean): time per unit of fitted work, by slot
    names, beta, _ = fits["tiles + cold + starts + slot + slab"]
    co = dict(zip(names, beta))
    for sc in scales:
        d = data[sc]
        work = co["tile"] * d["tiles"] + co["cold"] * d["cold"] + co["start"] * d["starts"]
        rate = (dur[sc] / np.maximum(work, 1e-9)).reshape(d["S"], 32, WAVES)
        rel = rate / rate.mean(axis=2, keepdims=True)
        say(f"R-MAT {sc}: time per unit of fitted work by wavefront slot, relative to the workgroup's mean: {np.round(rel.mean(axis=(0, 1)), 4).tolist()}"
            f" -> shares per mille that would level them: {np.round(1000 / rel.mean(axis=(0, 1)) / np.mean(1 / rel.mean(axis=(0, 1)))).astype(int).tolist()}")
        if sc != fit_scale:
            # no refit: the work terms and slot terms of R-MAT 24, one free offset per slab (a slab's level is its XCD's and its round's)
            pred = work + np.array([0.0] + [co[f"slot{j}"] for j in range(1, WAVES)])[np.arange(RANGES) % WAVES][None, :] * (work.mean() / (co["tile"] * data[fit_scale]["tiles"].mean()))
            res = dur[sc] - pred
            res = res - res.mean(axis=1, keepdims=True)
            within = dur[sc] - dur[sc].mean(axis=1, keepdims=True)
            say(f"R-MAT {sc} with R-MAT {fit_scale}'s coefficients (one offset per slab, nothing else refitted): within-slab R^2 "
                f"{1 - np.sum(res ** 2) / np.sum(within ** 2):.4f}, rms residual {np.sqrt(np.mean(res ** 2)):.2f} us of a mean range time {dur[sc].mean():.1f} us")
    with open(os.path.join(args.out, "range_cost_fit.txt"), "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
