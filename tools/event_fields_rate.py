#!/usr/bin/env python3
"""What the event-table field selection (ABEA_EV_FIELDS_*, include/abea.h) does to the raw-signal host entries on bench.py's
process_chain sample: the same 10 k reads of BASELINE configs[2] (permutation seed 777 of the 100 k-read batch, signals with seed 5),
built with bench.py's own generator settings and measured with its chain_bound().  Per selection, for event_db alone
(abea_events_batch_host_fields) and for the chain (abea_process_batch_host_fields): ms per call (median of --reps calls, the
selections alternated in one process), h2d / d2h bytes, the caller's flatten / scatter / wait ms, GPU-clock busy ms and the bound,
next to ctx.link_probe().  One JSON document on stdout and in --out.  Runs under rocprofv3 as well (--reps 1 for a kernel trace)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  first (through f5c_amd): the hardware-queue setting before the HIP runtime initialises
import numpy as np  # noqa: E402
from f5c_amd import abea, load_model_f32, synth  # noqa: E402

SELECTIONS = (("ALL", abea.EV_FIELDS_ALL), ("NO_STDV", abea.EV_FIELDS_NO_STDV), ("LAYOUT", abea.EV_FIELDS_LAYOUT))


def sample(n_reads):
    """bench.process_chain's sample: reads idx of configs[2] (make_batch(subset=) builds exactly those reads of the full batch)"""
    cfg = synth.CONFIGS["r9_100k_mixed"]
    k, model = load_model_f32(os.path.join(ROOT, "tests", "golden", "r9.4_450bps.6mer.f32"))
    idx = np.sort(np.random.default_rng(777).permutation(cfg["n_reads"])[:min(cfg["n_reads"], n_reads)])
    workers = max(1, min(16, bench.effective_cpus()))
    sub = synth.make_batch(cfg["n_reads"], model, k, seed=cfg["seed"], law=cfg["law"], workers=workers, subset=idx)
    sig, sp, ns, sc = synth.make_signals_flat(sub, seed=5, threads=max(2, bench.effective_cpus() - 2))
    return k, model, sub, sig, sp, ns, sc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    t0 = time.time()
    k, model, sub, sig, sp, ns, sc = sample(args.reads)
    gen_s = time.time() - t0
    ctx = abea.AbeaContext(model, k, device_id=0, verbosity=0, max_arena_bytes=150 << 30)
    link = ctx.link_probe()
    out = {"reads": int(len(ns)), "samples": int(ns.sum()), "signal_bytes_int16": int(ns.sum()) * 2, "gen_s": round(gen_s, 1),
           "reps": args.reps, "link_probe_gbs": link, "event_db_alone": {}, "process_chain": {}}
    for entry in ("event_db_alone", "process_chain"):
        call = ctx.events_view if entry == "event_db_alone" else ctx.process_view
        v = ctx.signal_view(sig, sp, ns, sc, batch=sub)
        for _, s in SELECTIONS:                                # warm: slots and pinned staging at their largest
            call(v, ev_fields=s)
            ctx.free_view(v)
        runs = {name: [] for name, _ in SELECTIONS}
        n_pairs = {}
        for rep in range(args.reps):
            order = SELECTIONS if rep % 2 == 0 else SELECTIONS[::-1]
            for name, s in order:
                t1 = time.perf_counter()
                call(v, ev_fields=s)
                ms = (time.perf_counter() - t1) * 1e3
                st = ctx.stats()
                runs[name].append((ms, st, int(v["n_events"].sum())))
                if entry == "process_chain":
                    n_pairs[name] = v["n_pairs"].copy()
                ctx.free_view(v)
        for name, s in SELECTIONS:
            ms_all = [r[0] for r in runs[name]]
            med = sorted(runs[name], key=lambda r: r[0])[len(ms_all) // 2]
            ms, st, n_ev = med
            host = {"flatten_signal": round(st["flatten_ms"], 1), "scatter_outputs": round(st["unflatten_ms"], 1),
                    "wait_for_gpu": round(st["wait_ms"], 1), "plan": round(st["plan_ms"], 1)}
            pcie = {"h2d": int(st["h2d_bytes"]), "d2h": int(st["d2h_bytes"])}
            e = {"ev_fields": s, "ms_per_call_median": round(statistics.median(ms_all), 1), "ms_per_call_all": [round(x, 1) for x in ms_all],
                 "events": n_ev, "pcie_bytes_per_call": pcie, "d2h_bytes_per_event": round(pcie["d2h"] / max(n_ev, 1), 3),
                 "host_ms_per_call": host, "gpu_busy_ms": round(st["gpu_busy_ms"], 1), "event_kernels_ms": round(st["event_ms"], 1),
                 "chunks": int(st["n_sub_batches"])}
            e.update(bench.chain_bound(ms, host, st["gpu_busy_ms"], pcie, link))
            out[entry][name] = e
        if entry == "process_chain":
            out[entry]["n_pairs_equal_across_selections"] = bool(all((n_pairs[name] == n_pairs["ALL"]).all() for name, _ in SELECTIONS))
    ctx.close()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
