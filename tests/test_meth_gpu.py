"""call-methylation, mode 0, on the GPU: abea_meth_batch_host (the job builder abea_meth_sites_kernel + abea_hmm_forward_kernel)
and abea_meth_format_batch, pinned to the restatement of calculate_methylation_for_read (tests/meth_restate.py) bit for bit, and
to the reference's printed single_read/meth.exp from the raw signal of its read."""
import os
import numpy as np
import pytest

import meth_restate as R
from test_meth_restate import check_text, load_cpg_model, read1_record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _restated(orc, cpg, kc, segs, pos, cigars, rc, read_len, events, maps, scal, epb, flags):
    """per read [(start, end, n_cpg, ll_m, ll_u)] and the skipped-group count, None for a refused read"""
    out, skipped = [], 0
    for i in range(len(segs)):
        if flags is not None and flags[i]:
            out.append([]); continue
        mstart = maps[i][:, 0] if maps[i] is not None else np.zeros(0, np.int32)
        groups, sk = R.plan_read(segs[i], int(pos[i]), cigars[i], bool(rc[i]), int(read_len[i]), mstart, len(events[i]), kc)
        if groups is None:
            return None, 0
        skipped += sk
        s = scal[i]
        sc = R.score_read(orc, groups, events[i], (s["scale"], s["shift"], s["var"], s["log_var"]), cpg, kc, bool(rc[i]), epb[i])
        out.append([(g["start"], g["end"], g["n_cpg"], m, u) for g, (m, u) in zip(groups, sc)])
    return out, skipped


def _same_sites(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), (i, len(g), len(w))
        if not len(w):
            continue
        w = np.array(w, dtype=[("s", "<i4"), ("e", "<i4"), ("n", "<i4"), ("m", "<f4"), ("u", "<f4")])
        assert (g["start_position"] == w["s"]).all() and (g["end_position"] == w["e"]).all() and (g["n_cpg"] == w["n"]).all(), i
        assert (g["strands_scored"] == 1).all()
        assert (g["ll_methylated"].view(np.uint32) == w["m"].view(np.uint32)).all(), i
        assert (g["ll_unmethylated"].view(np.uint32) == w["u"].view(np.uint32)).all(), i


@pytest.mark.gpu
def test_read1_from_raw_signal_to_text(ctx, orc, r9):
    """read1's signal -> abea_process_batch_host -> abea_meth_batch_host on the synthetic segment: the restatement bit for bit on
    the device's own map and scalings, and single_read/meth.exp within the print rule of the CPU pin"""
    from f5c_amd import abea
    k, model = r9
    kc, cpg = load_cpg_model()
    g = np.load(os.path.join(GOLDEN, "read1_events.npz"))
    sig = g["signal"].astype(np.float32)
    seq = g["seq"].tobytes()
    b = dict(reads=g["seq"].copy(), read_len=np.array([len(seq)], np.int32), read_ptr=np.array([0], np.int64))
    v = ctx.signal_view(sig, np.array([0], np.int64), np.array([len(sig)], np.int64), g["scaling"].reshape(1, 3), batch=b)
    ctx.process_view(v, ev_fields=abea.EV_FIELDS_NO_STDV)
    try:
        assert int(v["read_stat_flag"][0]) == 0
        r = read1_record()
        sites = ctx.meth_batch([r["segment"]], [r["pos"]], [r["cigar"]], [r["rc"]], v["read_len"], v["ev_pp"], v["map_pp"],
                               v["scalings"], v["events_per_base"], cpg, kc, read_stat_flag=v["read_stat_flag"], n_events=v["n_events"])
        st = ctx.stats()
        ev = ctx.view_events(v, 0)
        m = ctx.view_map(v, 0, len(seq) - k + 1)
    finally:
        ctx.free_view(v)
    assert len(sites[0]) == 45 and st["meth_groups"] == 45 and st["meth_groups_skipped"] == 0 and st["meth_ms"] > 0
    want, _ = _restated(orc, cpg, kc, [r["segment"]], [r["pos"]], [r["cigar"]], [r["rc"]], [len(seq)], [ev], [m], v["scalings"],
                        v["events_per_base"], None)
    _same_sites(sites, want)
    text = abea.meth_format([r["contig"]], [r["name"]], [r["rc"]], [r["segment"]], [r["pos"]], sites, k, header=True)
    check_text(text, r["text"])


IUPAC = "ACGTMRWSYKVHDBNacgtn"


def synth_reads(n, seed, k=6):
    """Reads with random CIGARs (M, I, D, soft and hard clips), events, maps holding -1 runs and segments with CpGs, IUPAC codes
    and lower case; both strands"""
    rng = np.random.default_rng(seed)
    R_ = dict(segs=[], pos=[], cigars=[], rc=[], read_len=[], events=[], maps=[], scal=[], epb=[])
    from f5c_amd.types import EVENT_DT, SCAL_DT
    for i in range(n):
        L = int(rng.integers(300, 3000))
        ops, used = [], 0
        if rng.random() < 0.5:
            ops.append((int(rng.integers(1, 30)), 5))
        if rng.random() < 0.7:
            c = int(rng.integers(1, 60)); ops.append((c, 4)); used += c
        while used < L - 40:
            c = int(rng.integers(3, 40)); ops.append((c, int(rng.choice([0, 0, 0, 7, 8])))); used += c
            r = rng.random()
            if r < 0.3:
                c = int(rng.integers(1, 6)); ops.append((c, 1)); used += c
            elif r < 0.6:
                ops.append((int(rng.integers(1, 6)), 2))
        if rng.random() < 0.7:
            ops.append((max(1, L - used), 4))
        if rng.random() < 0.5:
            ops.append((int(rng.integers(1, 30)), 5))
        cigar = np.array([(c << 4) | o for c, o in ops], dtype=np.uint32)
        span = R.ref_span(cigar)
        seg = list(rng.choice(list("ACGT"), size=span + 1, p=[0.3, 0.2, 0.2, 0.3]))
        for j in rng.choice(span + 1, size=max(1, span // 50)):
            seg[j] = str(rng.choice(list(IUPAC)))
        seg = "".join(seg)
        E = int(L * rng.uniform(1.5, 2.5))
        ev = np.zeros(E, dtype=EVENT_DT)
        ev["mean"] = rng.uniform(60, 120, E).astype(np.float32)
        K = L - k + 1
        starts = np.sort(rng.integers(0, E, K)).astype(np.int32)
        mp = np.stack([starts, starts], axis=1).astype(np.int32)
        holes = rng.random(K) < 0.1
        for _ in range(int(rng.integers(0, 3))):                       # runs of unmapped k-mers
            a = int(rng.integers(0, K)); holes[a:a + int(rng.integers(5, 1500))] = True
        mp[holes] = -1
        if i % 5 == 3 and K > 1300:                                    # no event within 1000 k-mers: bounds of -1, skipped and counted
            mp[:1100] = -1
        s = np.zeros(1, dtype=SCAL_DT)[0]
        s["scale"], s["shift"], s["var"] = rng.uniform(0.9, 1.1), rng.uniform(-5, 5), rng.uniform(1, 2)
        s["log_var"] = np.log(s["var"])
        for key, val in (("segs", seg), ("pos", int(rng.integers(0, 100000))), ("cigars", cigar), ("rc", int(rng.random() < 0.5)),
                         ("read_len", L), ("events", ev), ("maps", mp), ("scal", s), ("epb", float(rng.uniform(1.5, 2.5)))):
            R_[key].append(val)
    R_["scal"] = np.array(R_["scal"], dtype=SCAL_DT)
    return R_


def _run(ctx, S, cpg, kc, flags=None):
    return ctx.meth_batch(S["segs"], S["pos"], S["cigars"], S["rc"], S["read_len"], S["events"], S["maps"], S["scal"], S["epb"], cpg, kc,
                          read_stat_flag=flags)


@pytest.mark.gpu
def test_synthetic_reads_match_the_restatement(ctx, orc):
    """both strands, clips, indels, IUPAC codes and lower case, -1 runs in the map (skipped groups counted), flagged and empty reads"""
    kc, cpg = load_cpg_model()
    S = synth_reads(40, seed=11)
    # a read with no CpG, an empty read, a read shorter than k, a group cut at the segment's end, a group with span > 200
    S["segs"][1] = S["segs"][1].replace("C", "A").replace("c", "a").replace("S", "A").replace("Y", "A").replace("B", "A")
    S["segs"][2] = ""; S["read_len"][2] = 0; S["cigars"][2] = np.zeros(0, np.uint32); S["events"][2] = S["events"][2][:0]; S["maps"][2] = None
    S["read_len"][3] = 4; S["maps"][3] = None
    S["segs"][4] = S["segs"][4][:-3] + "ACG"
    S["segs"][5] = S["segs"][5][:100] + "CGAAAACGTT" * 30 + S["segs"][5][400:]
    flags = np.zeros(40, np.int32); flags[6] = 1; flags[7] = 4
    got = _run(ctx, S, cpg, kc, flags)
    st = ctx.stats()
    want, skipped = _restated(orc, cpg, kc, S["segs"], S["pos"], S["cigars"], S["rc"], S["read_len"], S["events"], S["maps"], S["scal"],
                              S["epb"], flags)
    _same_sites(got, want)
    assert len(got[1]) == 0 and len(got[2]) == 0 and len(got[3]) == 0 and len(got[6]) == 0 and len(got[7]) == 0
    assert sum(len(x) for x in got) > 100 and skipped > 0
    assert st["meth_groups_skipped"] == skipped and st["meth_groups"] == sum(len(x) for x in got)
    assert st["n_reads_skipped"] == 2
    # chunks of 1 and 7 reads: the same bytes
    for c in ("1", "7"):
        os.environ["ABEA_METH_CHUNK_READS"] = c
        try:
            again = _run(ctx, S, cpg, kc, flags)
        finally:
            del os.environ["ABEA_METH_CHUNK_READS"]
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again, got)), c
        assert ctx.stats()["n_sub_batches"] >= (38 if c == "1" else 6)


@pytest.mark.gpu
def test_refusals_and_empty_batch(ctx):
    from f5c_amd import abea
    kc, cpg = load_cpg_model()
    assert ctx.meth_batch([], [], [], [], [], [], [], np.zeros(0, dtype=abea.SCAL_DT), [], cpg, kc) == []
    S = synth_reads(6, seed=5)
    S["cigars"][3] = np.concatenate([S["cigars"][3][:2], np.array([(50 << 4) | 3], np.uint32), S["cigars"][3][2:]])   # N: ref skip
    with pytest.raises(abea.AbeaError, match=r"\(-1\)"):
        _run(ctx, S, cpg, kc)
    S = synth_reads(6, seed=5)
    S["segs"][2] = S["segs"][2][:50] + "X" + S["segs"][2][51:]          # no IUPAC code
    with pytest.raises(abea.AbeaError, match=r"\(-1\)"):
        _run(ctx, S, cpg, kc)
    S = synth_reads(6, seed=5)                                            # the context is unharmed
    assert sum(len(x) for x in _run(ctx, S, cpg, kc)) > 0


@pytest.mark.gpu
def test_two_device_context_on_one_gpu(orc, r9):
    from f5c_amd import abea
    k, model = r9
    kc, cpg = load_cpg_model()
    S = synth_reads(24, seed=3)
    with abea.AbeaContext(model, k, device_ids=[0, 0], max_arena_bytes=1 << 30) as c2:
        got = _run(c2, S, cpg, kc)
        st = c2.stats()
    want, skipped = _restated(orc, cpg, kc, S["segs"], S["pos"], S["cigars"], S["rc"], S["read_len"], S["events"], S["maps"], S["scal"],
                              S["epb"], None)
    _same_sites(got, want)
    assert st["n_devices"] == 2 and st["meth_groups_skipped"] == skipped


def ecoli_records(k):
    """every mapped record of reads.sorted.bam whose read has an event table in ecoli_events.npz, in file order, with its synthetic
    segment: meth.exp holds rows of secondary and mapq-0 records too, so it was printed with every mapped record kept
    (f5cio.c:550-610 under --secondary=yes --min-mapq=0)"""
    g = dict(np.load(os.path.join(GOLDEN, "meth_golden.npz")))
    z = np.load(os.path.join(GOLDEN, "ecoli_events.npz"))
    names = {str(r): i for i, r in enumerate(z["read_id"])}
    rows = {}
    for j, r in enumerate(g["ecoli_row_read"]):
        rows.setdefault(str(r), []).append(j)
    recs = []
    for q in range(len(g["ecoli_name"])):
        name, f = str(g["ecoli_name"][q]), int(g["ecoli_flag"][q])
        if f & 4 or name not in names:
            continue
        pos = int(g["ecoli_pos"][q])
        cig = g["ecoli_cigar"][g["ecoli_cigar_ptr"][q]:g["ecoli_cigar_ptr"][q + 1]]
        contig, span = str(g["ecoli_contigs"][g["ecoli_tid"][q]]), R.ref_span(cig)
        wins = [(int(g["ecoli_row_start"][j]) - k + 1 - pos, str(g["ecoli_row_seq"][j])) for j in rows.get(name, [])
                if str(g["ecoli_row_contig"][j]) == contig and pos <= int(g["ecoli_row_start"][j]) <= pos + span]
        recs.append(dict(read=names[name], name=name, pos=pos, cigar=cig, rc=bool(f & 16), contig=contig,
                         segment=R.synthetic_segment(span + 1, wins)))
    want = list(zip(g["ecoli_row_contig"].tolist(), g["ecoli_row_start"].tolist(), g["ecoli_row_end"].tolist(),
                    g["ecoli_row_read"].tolist(), g["ecoli_row_ncpg"].tolist(), g["ecoli_row_seq"].tolist()))
    return recs, z, want


@pytest.mark.gpu
def test_ecoli_all_records(ctx, orc, r9):
    """The 111 reads' events aligned and scaled on the device, every mapped record called: {contig, start, end, read_name, n_cpg,
    sequence} and the row order equal meth.exp's 20 630 rows; the scores equal the restatement's bit for bit on the device's maps
    and scalings (the printed scores cannot be pinned: the window bases outside the printed columns are unknown)."""
    from f5c_amd import abea
    from f5c_amd.types import EVENT_DT, SCAL_DT
    k, model = r9
    kc, cpg = load_cpg_model()
    recs, z, want = ecoli_records(k)
    n = len(z["read_id"])
    seqs, evs = [], []
    for i in range(n):
        a, b = int(z["ev_ptr"][i]), int(z["ev_ptr"][i + 1])
        ev = np.zeros(b - a, dtype=EVENT_DT)
        ev["mean"] = z["mean"][a:b]
        evs.append(ev)
        seqs.append(z["seq"][int(z["seq_ptr"][i]):int(z["seq_ptr"][i + 1])].tobytes())
    sc = np.zeros(n, dtype=SCAL_DT)
    sc["scale"], sc["shift"] = z["scale"], z["shift"]
    _, _, _, S = ctx.align_db_host(seqs, evs, sc, scaling=True, want_pairs=False)
    assert int((S["read_stat_flag"] != 0).sum()) == 0
    ri = [r["read"] for r in recs]
    sites = ctx.meth_batch([r["segment"] for r in recs], [r["pos"] for r in recs], [r["cigar"] for r in recs], [r["rc"] for r in recs],
                           [len(seqs[i]) for i in ri], [evs[i] for i in ri], [S["base_to_event_map"][i] for i in ri], S["scalings"][ri],
                           S["events_per_base"][ri], cpg, kc, read_stat_flag=S["read_stat_flag"][ri])
    text = abea.meth_format([r["contig"] for r in recs], [r["name"] for r in recs], [r["rc"] for r in recs], [r["segment"] for r in recs],
                            [r["pos"] for r in recs], sites, k)
    got = [l.split("\t") for l in text.splitlines()]
    got = [(a[0], int(a[1]), int(a[2]), a[3], int(a[8]), a[9]) for a in got]
    assert len(got) == 20630 and got == want
    # scores: the restatement on the device's maps and scalings
    for r, s in zip(recs, sites):
        i = r["read"]
        groups, skipped = R.plan_read(r["segment"], r["pos"], r["cigar"], r["rc"], len(seqs[i]), S["base_to_event_map"][i][:, 0],
                                      len(evs[i]), kc, fast=True)
        t = S["scalings"][i]
        res = R.score_read(orc, groups, evs[i], (t["scale"], t["shift"], t["var"], t["log_var"]), cpg, kc, r["rc"], S["events_per_base"][i])
        _same_sites([s], [[(g["start"], g["end"], g["n_cpg"], m, u) for g, (m, u) in zip(groups, res)]])


@pytest.mark.gpu
def test_shim_from_a_plain_gpp_caller(ctx, r9, tmp_path):
    """abea_f5c_meth (include/abea_f5c_shim.h) from a g++ program: the same sites as the library entry, the same text as meth_format"""
    import subprocess
    from f5c_amd import abea
    k, model = r9
    kc, cpg = load_cpg_model()
    S = synth_reads(12, seed=21)
    flags = np.zeros(12, np.int32); flags[4] = 2
    want = _run(ctx, S, cpg, kc, flags)
    with open(str(tmp_path / "in.bin"), "wb") as f:
        f.write(np.array([12, k, len(model)], np.int32).tobytes())
        f.write(np.ascontiguousarray(model).tobytes()); f.write(np.ascontiguousarray(cpg).tobytes())
        for i in range(12):
            seg = S["segs"][i].encode()
            f.write(np.array([S["pos"][i], S["rc"][i], S["read_len"][i], len(S["cigars"][i]), len(seg), len(S["events"][i]), flags[i], 0],
                             np.int32).tobytes())
            f.write(S["cigars"][i].astype(np.uint32).tobytes()); f.write(seg)
            f.write(S["events"][i]["mean"].astype(np.float32).tobytes()); f.write(S["maps"][i][:, 0].astype(np.int32).tobytes())
            f.write(S["scal"][i:i + 1].tobytes()); f.write(np.array([S["epb"][i]], np.float64).tobytes())
    exe = str(tmp_path / "meth_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O2", os.path.join(ROOT, "tests", "meth_driver.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "f5c_amd"), "-labea_hip", "-Wl,-rpath," + os.path.join(ROOT, "f5c_amd")])
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out")])
    raw = open(str(tmp_path / "out.sites"), "rb").read()
    o = 0
    for i in range(12):
        ns = int(np.frombuffer(raw, np.int32, 1, o)[0]); o += 4
        got = np.frombuffer(raw, abea.SITE_DT, ns, o); o += ns * abea.SITE_DT.itemsize
        assert got.tobytes() == want[i].tobytes(), i
    assert o == len(raw) and sum(len(w) for w in want) > 0 and len(want[4]) == 0
    text = abea.meth_format(["ctg"] * 12, ["read%d" % i for i in range(12)], S["rc"], S["segs"], S["pos"], want, k, version=2, header=True,
                            read_stat_flag=flags)
    assert open(str(tmp_path / "out.tsv")).read() == text
