#!/usr/bin/env python3
"""Rate of call-methylation, mode 0 (abea_meth_batch_host): about 10 k synthetic reads of 1-20 kb with random CpG-bearing reference
segments, CIGARs (M / = / X runs, insertions, deletions, clips) and base_to_event_maps with unmapped runs, both strands.  Reads are
drawn from --templates distinct synthetic reads (each with its own events, map, CIGAR and segment; a template's arrays are shared by
the reads that use it, which the library does not see), so that host memory stays small.

Reports, as one JSON document on stdout and in --out: groups/s and jobs/s of the entry (median of --reps calls), its time split
(the job builder's two passes and the forward kernel on the GPU clock, copies' bytes, the caller-thread flatten / job planning /
site loops) and, on --sample reads, the single-thread rate of the restatement (tests/meth_restate.py: Python planning + the C
oracle's profile_hmm_score), with a bit-exact check of the entry's sites against it.  Runs under rocprofv3 as well (--reps 1)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import f5c_amd  # noqa: E402,F401  first: the hardware-queue setting before the HIP runtime initialises
import numpy as np  # noqa: E402
from f5c_amd import abea, load_model_f32  # noqa: E402
from f5c_amd.types import EVENT_DT, SCAL_DT  # noqa: E402


def template(rng, k):
    L = int(rng.integers(1000, 20001))
    ops, used = [], 0
    if rng.random() < 0.5:
        ops.append((int(rng.integers(1, 50)), 5))
    c = int(rng.integers(1, 200)); ops.append((c, 4)); used += c
    while used < L - 200:
        c = int(rng.integers(3, 40)); ops.append((c, int(rng.choice([0, 0, 0, 7, 8])))); used += c
        r = rng.random()
        if r < 0.3:
            c = int(rng.integers(1, 6)); ops.append((c, 1)); used += c
        elif r < 0.6:
            ops.append((int(rng.integers(1, 6)), 2))
    ops.append((max(1, L - used), 4))
    cigar = np.array([(c << 4) | o for c, o in ops], dtype=np.uint32)
    span = int(sum(c for c, o in ops if o in (0, 2, 7, 8)))
    seg = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=span + 1, p=[0.3, 0.2, 0.2, 0.3]).tobytes()
    E = int(L * rng.uniform(1.6, 2.4))
    ev = np.zeros(E, dtype=EVENT_DT)
    ev["mean"] = rng.uniform(60, 120, E).astype(np.float32)
    K = L - k + 1
    starts = np.sort(rng.integers(0, E, K)).astype(np.int32)
    mp = np.stack([starts, starts], axis=1)
    mp[rng.random(K) < 0.1] = -1
    return dict(L=L, cigar=cigar, seg=seg, ev=ev, map=np.ascontiguousarray(mp, dtype=np.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--templates", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sample", type=int, default=20, help="reads scored by the restatement too (0 = none)")
    ap.add_argument("--seed", type=int, default=8)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    k, model = load_model_f32(os.path.join(ROOT, "tests", "golden", "r9.4_450bps.6mer.f32"))
    from test_meth_restate import load_cpg_model
    kc, cpg = load_cpg_model()
    rng = np.random.default_rng(args.seed)
    t0 = time.perf_counter()
    T = [template(rng, k) for _ in range(args.templates)]
    pick = rng.integers(0, len(T), args.reads)
    rc = (rng.random(args.reads) < 0.5).astype(np.uint8)
    pos = rng.integers(0, 4_000_000, args.reads).astype(np.int32)
    sc = np.zeros(args.reads, dtype=SCAL_DT)
    sc["scale"] = rng.uniform(0.9, 1.1, args.reads); sc["shift"] = rng.uniform(-5, 5, args.reads)
    sc["var"] = rng.uniform(1, 2, args.reads); sc["log_var"] = np.log(sc["var"])
    epb = rng.uniform(1.6, 2.4, args.reads)
    ev_pp = np.array([T[t]["ev"].ctypes.data for t in pick], dtype=np.uint64)
    n_ev = np.array([len(T[t]["ev"]) for t in pick], dtype=np.uint64)
    map_pp = np.array([T[t]["map"].ctypes.data for t in pick], dtype=np.uint64)
    segs = [T[t]["seg"] for t in pick]
    cigars = [T[t]["cigar"] for t in pick]
    read_len = np.array([T[t]["L"] for t in pick], dtype=np.int32)
    gen_s = time.perf_counter() - t0
    out = dict(reads=args.reads, templates=args.templates, bases=int(read_len.sum()), ref_bases=int(sum(len(s) for s in segs)),
               events=int(n_ev.sum()), generate_s=round(gen_s, 2))
    with abea.AbeaContext(model, k, device_id=0, max_arena_bytes=8 << 30) as ctx:
        def call():
            t = time.perf_counter()
            s = ctx.meth_batch(segs, pos, cigars, rc, read_len, ev_pp, map_pp, sc, epb, cpg, kc, n_events=n_ev)
            return s, (time.perf_counter() - t) * 1e3, ctx.stats()
        sites, _, _ = call()                                     # warm-up: code objects, pinned staging, worker pool
        runs = [call() for _ in range(args.reps)]
        ms = [r[1] for r in runs]
        st = runs[len(runs) // 2][2]
        same = all(all(a.tobytes() == b.tobytes() for a, b in zip(r[0], sites)) for r in runs)
        groups = int(st["meth_groups"])
        med = statistics.median(ms)
        out.update(call_ms=[round(x, 2) for x in ms], call_ms_median=round(med, 2), groups=groups, jobs=2 * groups,
                   groups_skipped=int(st["meth_groups_skipped"]), groups_per_s=round(groups / med * 1e3), jobs_per_s=round(2 * groups / med * 1e3),
                   repeat_identical=same,
                   split_ms=dict(total=round(st["total_ms"], 2), site_kernel=round(st["meth_ms"] - st["hmm_ms"], 2),
                                 forward_kernel=round(st["hmm_ms"], 2), flatten=round(st["flatten_ms"], 2), plan_jobs=round(st["plan_ms"], 2),
                                 sites=round(st["unflatten_ms"], 2),
                                 copies_and_rest=round(st["total_ms"] - st["meth_ms"] - st["flatten_ms"] - st["plan_ms"] - st["unflatten_ms"], 2)),
                   h2d_bytes=int(st["h2d_bytes"]), d2h_bytes=int(st["d2h_bytes"]), chunks=int(st["n_sub_batches"]),
                   host_threads=int(st["host_threads"]))
    if args.sample:
        import meth_restate as R
        from oracle import orc
        orc.lib()
        t = time.perf_counter()
        n_groups, exact = 0, True
        for i in range(args.sample):
            tp = T[pick[i]]
            groups, _ = R.plan_read(tp["seg"].decode(), int(pos[i]), tp["cigar"], bool(rc[i]), tp["L"], tp["map"][:, 0], len(tp["ev"]), kc,
                                    fast=True)
            s = sc[i]
            res = R.score_read(orc, groups, tp["ev"], (s["scale"], s["shift"], s["var"], s["log_var"]), cpg, kc, bool(rc[i]), epb[i])
            n_groups += len(groups)
            g = sites[i]
            exact &= len(g) == len(groups) and all(
                (int(a["start_position"]), int(a["n_cpg"])) == (b["start"], b["n_cpg"]) and
                np.float32(a["ll_methylated"]).view(np.uint32) == m.view(np.uint32) and
                np.float32(a["ll_unmethylated"]).view(np.uint32) == u.view(np.uint32) for a, b, (m, u) in zip(g, groups, res))
        dt = time.perf_counter() - t
        out.update(restatement=dict(reads=args.sample, groups=n_groups, seconds=round(dt, 2), groups_per_s=round(n_groups / dt),
                                    bit_exact=bool(exact)))
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if out["repeat_identical"] and out.get("restatement", {}).get("bit_exact", True) else 1


if __name__ == "__main__":
    sys.exit(main())
