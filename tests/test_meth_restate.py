"""CPU pin of call-methylation (mode 0) on read1 of test/ecoli_2kb_region/single_read.

The restatement of calculate_methylation_for_read (tests/meth_restate.py), given the oracle's base_to_event_map (orc.scaling_single)
and the read's BAM record (tests/golden/meth_golden.npz, minted by make_meth_golden.py), on a synthetic segment that holds the
printed m_seq windows over a filler of 'A', must reproduce all 90 profile_hmm_score arguments of meth_input.exp and the 45 rows of
single_read/meth.exp.  abea_meth_format_batch (host-only) must print the file, header included, from the oracle's scores: on every
line but the one test_hmm_pin.py knows sits at a %.2f rounding edge, where the score columns may differ by 0.01."""
import os
import numpy as np
import pytest

import meth_restate as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_cpg_model():
    from f5c_amd.model import _finish
    tab = np.fromfile(os.path.join(GOLDEN, "r9.4_450bps.cpg.6mer.f32"), dtype=np.float32).reshape(-1, 2)
    return 6, _finish(tab[:, 0], tab[:, 1])


def read1_record():
    g = np.load(os.path.join(GOLDEN, "meth_golden.npz"))
    pos, flag = int(g["read1_pos"][0]), int(g["read1_flag"][0])
    cigar = g["read1_cigar"][g["read1_cigar_ptr"][0]:g["read1_cigar_ptr"][1]]
    # faidx_fetch_seq(pos, bam_endpos) includes its end (f5cio.c:622): one base more than the record spans
    seg = R.synthetic_segment(R.ref_span(cigar) + 1, [(p - pos, s) for p, s in zip(g["read1_win_pos"], g["read1_win_seq"])])
    return dict(pos=pos, rc=bool(flag & 16), cigar=cigar, segment=seg, contig=str(g["read1_contigs"][g["read1_tid"][0]]),
                name=str(g["read1_name"][0]), text=str(g["read1_meth_exp"]))


def read1_scaled(orc, r9, single_read):
    k, model = r9
    seq, ev = single_read["seq"], single_read["events"]
    scale, shift = orc.estimate_scalings(seq, model, k, ev)
    pairs, _ = orc.align(seq, ev, model, k, scale, shift)
    return orc.scaling_single(pairs, seq, ev, model, k, scale, shift)


def check_text(got, want):
    """equal line by line, except score columns within 0.01 on the one line at a %.2f rounding edge"""
    gl, wl = got.splitlines(), want.splitlines()
    assert len(gl) == len(wl)
    loose = 0
    for a, b in zip(gl, wl):
        if a == b:
            continue
        fa, fb = a.split("\t"), b.split("\t")
        sc = [i for i in range(len(fa)) if fa[i] != fb[i]]
        assert fa[:4] == fb[:4] and fa[7:] == fb[7:], (a, b)
        assert all(abs(float(fa[i]) - float(fb[i])) <= 0.0100001 for i in sc), (a, b)
        loose += 1
    assert loose <= 1, loose


def test_restatement_reproduces_meth_input(orc, r9, single_read):
    k = r9[0]
    rec = read1_scaled(orc, r9, single_read)
    r = read1_record()
    assert r["rc"] and r["pos"] == 10
    groups, skipped = R.plan_read(r["segment"], r["pos"], r["cigar"], r["rc"], len(single_read["seq"]),
                                  rec["base_to_event_map"]["start"], len(single_read["events"]), k)
    hm = np.load(os.path.join(GOLDEN, "single_read_meth.npz"))
    assert skipped == 0 and len(groups) == 45
    for i, g in enumerate(groups):
        u, m = hm["args"][2 * i], hm["args"][2 * i + 1]
        assert (g["m_seq"], g["m_rc_seq"]) == (hm["m_seq"][2 * i], hm["m_rc_seq"][2 * i])
        assert (g["mm_seq"], g["mm_rc_seq"]) == (hm["m_seq"][2 * i + 1], hm["m_rc_seq"][2 * i + 1])
        assert (g["e1"], g["e2"], g["stride"], 1) == tuple(u) == tuple(m)
        assert g["n_cpg"] == hm["exp_num_cpgs"][i]


def test_restatement_and_formatter_reproduce_meth_exp(orc, r9, single_read):
    from f5c_amd import abea
    k = r9[0]
    kc, cpg = load_cpg_model()
    rec = read1_scaled(orc, r9, single_read)
    r = read1_record()
    groups, _ = R.plan_read(r["segment"], r["pos"], r["cigar"], r["rc"], len(single_read["seq"]),
                            rec["base_to_event_map"]["start"], len(single_read["events"]), k)
    sc = rec["scalings"]
    scores = R.score_read(orc, groups, single_read["events"], (sc["scale"], sc["shift"], sc["var"], sc["log_var"]), cpg, kc,
                          r["rc"], rec["events_per_base"])
    sites = np.array([(g["start"], g["end"], g["n_cpg"], 1, m, u) for g, (m, u) in zip(groups, scores)], dtype=abea.SITE_DT)
    text = abea.meth_format([r["contig"]], [r["name"]], [r["rc"]], [r["segment"]], [r["pos"]], [sites], k, version=1, header=True)
    check_text(text, r["text"])
    rows = [(int(s["start_position"]), int(s["end_position"]), int(s["n_cpg"]), s["ll_methylated"], s["ll_unmethylated"]) for s in sites]
    assert text == R.HEADER[1] + R.format_rows(r["contig"], r["name"], r["rc"], r["segment"], r["pos"], rows, k)
    # version 2 adds the strand column; the clip window drops rows outside [clip_start, clip_end)
    v2 = abea.meth_format([r["contig"]], [r["name"]], [r["rc"]], [r["segment"]], [r["pos"]], [sites], k, version=2, header=True)
    assert v2 == R.HEADER[2] + R.format_rows(r["contig"], r["name"], r["rc"], r["segment"], r["pos"], rows, k, version=2)
    lo, hi = int(sites["start_position"][5]), int(sites["end_position"][30])
    clip = abea.meth_format([r["contig"]], [r["name"]], [r["rc"]], [r["segment"]], [r["pos"]], [sites], k, clip_start=lo, clip_end=hi)
    assert clip == R.format_rows(r["contig"], r["name"], r["rc"], r["segment"], r["pos"], rows, k, clip_start=lo, clip_end=hi)
    assert len(clip.splitlines()) == 25
    # a flagged read prints nothing
    assert abea.meth_format([r["contig"]], [r["name"]], [r["rc"]], [r["segment"]], [r["pos"]], [sites], k, read_stat_flag=[1]) == ""


def test_restatement_quirks():
    """get_next_event never visits its stop index (index 0 is never searched backwards, map_size - 1 never forwards); a record
    whose first and last event are equal is dropped; an N op refuses the read"""
    k, L = 6, 40                                        # kept read positions 6..33, map_size 35
    b2e = np.full(L - k + 1, -1, dtype=np.int32)
    b2e[0], b2e[20], b2e[30] = 3, 5, 8
    rec = R.event_alignment_record(100, [L << 4], False, L, b2e, k)
    assert [e for _, e in rec] == [5] * 24 + [8] * 4   # positions 6..19 find 5 forwards, never 3 at index 0
    assert [r for r, _ in rec] == list(range(106, 134))
    b2e[:] = -1
    b2e[0], b2e[L - k] = 3, 9
    assert R.event_alignment_record(100, [L << 4], False, L, b2e, k) == []      # all -1: first == last, dropped (meth.c:176-183)
    assert R.event_alignment_record(100, [(10 << 4) | 3, (L << 4)], False, L, b2e, k) is None
    assert R.event_alignment_record_np(100, [(10 << 4) | 3, (L << 4)], False, L, b2e, k) is None


def test_restatement_reproduces_the_rows_of_meth_exp(orc, r9):
    """All mapped records of reads.sorted.bam on the oracle's maps: the 20 630 rows of meth.exp, positions, read, n_cpg, the
    sequence column and the order (the scores are not pinned: the synthetic segments know only the printed columns)"""
    from test_meth_gpu import ecoli_records
    from f5c_amd.types import EVENT_DT
    k, model = r9
    recs, z, want = ecoli_records(k)
    maps = {}
    for i in sorted({r["read"] for r in recs}):
        a, b = int(z["ev_ptr"][i]), int(z["ev_ptr"][i + 1])
        ev = np.zeros(b - a, dtype=EVENT_DT)
        ev["mean"] = z["mean"][a:b]
        seq = z["seq"][int(z["seq_ptr"][i]):int(z["seq_ptr"][i + 1])].tobytes()
        scale, shift = float(z["scale"][i]), float(z["shift"][i])
        pairs, _ = orc.align(seq, ev, model, k, scale, shift)
        rec = orc.scaling_single(pairs, seq, ev, model, k, scale, shift)
        assert rec["flag"] == 0
        maps[i] = (rec["base_to_event_map"]["start"], len(seq), len(ev))
    got = []
    for r in recs:
        m, L, E = maps[r["read"]]
        groups, _ = R.plan_read(r["segment"], r["pos"], r["cigar"], r["rc"], L, m, E, k, fast=True)
        got += [(r["contig"], g["start"], g["end"], r["name"], g["n_cpg"], r["segment"][g["start"] - r["pos"] - k + 1:g["end"] - r["pos"] + k])
                for g in groups]
    assert len(got) == 20630 and got == want


def test_numpy_record_equals_the_walk(orc, r9, single_read):
    """event_alignment_record_np (used for the 143 records above) = the literal walk, on read1 and on a map with -1 runs"""
    k = r9[0]
    rec = read1_scaled(orc, r9, single_read)
    r = read1_record()
    m = rec["base_to_event_map"]["start"].copy()
    L = len(single_read["seq"])
    for mp in (m, np.where((np.arange(len(m)) % 1700) < 1200, -1, m)):
        for rc in (True, False):
            assert R.event_alignment_record_np(r["pos"], r["cigar"], rc, L, mp, k) == R.event_alignment_record(r["pos"], r["cigar"], rc, L, mp, k)
