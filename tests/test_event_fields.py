"""Event-table field selection of the raw-signal host entries (abea_events_batch_host_fields / abea_process_batch_host_fields,
include/abea.h; the abea_f5c_*_fields shim calls): ABEA_EV_FIELDS_ALL hands back start, length, mean and stdv of every event as
today, NO_STDV start, length and mean (call-methylation reads the means, src/hmm.c:85), LAYOUT start and length (resquiggle reads
nothing else, src/resquiggle.c:373-380).  Only the selected fields cross PCIe (12 / 8 / 4 bytes per event).  Checked here:
  * the selected fields are bit-equal to the ALL run and to the oracle's getevents, the others and event_t's tail padding are zero
    bits, for DNA and RNA (reversed) tables through both entries, with many chunks rotating through few slots;
  * every other output of the process entry is bit-identical to the ALL run (the alignment reads the means in HBM);
  * the bytes that come down follow the selection;
  * overflowed tables (redone after the pipeline) follow the selection, and so does a two-device context;
  * any other selection is refused before any work, with no table handed back;
  * the reference's printed table of its single test read (tests/golden/read1_events.npz) through both entries;
  * a plain g++ resquiggle-shaped caller prints the same TSV / PAF from LAYOUT tables as from whole ones."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest

from test_chain_pipeline import _batch_and_signals, _oracle_chain
from test_process_chain import _dump, _raw_reads
from test_rna_events import rna_like_reads, rna_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ALL, NO_STDV, LAYOUT = 0, 1, 2
SELECTIONS = (ALL, NO_STDV, LAYOUT)
FIELDS = {ALL: ("start", "length", "mean", "stdv"), NO_STDV: ("start", "length", "mean"), LAYOUT: ("start", "length")}
WIDTH = {ALL: 12, NO_STDV: 8, LAYOUT: 4}                     # bytes per event over PCIe
ZERO_WORDS = {ALL: (5,), NO_STDV: (4, 5), LAYOUT: (3, 4, 5)}  # event_t as 6 uint32: start lo/hi, length, mean, stdv, padding


def _pipeline_env(monkeypatch):
    """48 reads, 3 slots, chunks of 300 k samples: at least 5 chunks rotate (as test_tables_cross_pcie_in_either_form_by_either_mover)"""
    monkeypatch.setenv("ABEA_CHAIN_SLOTS", "3")
    monkeypatch.setenv("ABEA_CHAIN_CHUNK_SAMPLES", str(300_000))
    monkeypatch.setenv("ABEA_CHAIN_CHUNK_READS", "5")


def _rna_batch(n, seed):
    seqs, sigs, sc = rna_like_reads(n, seed)
    ns = np.array([len(s) for s in sigs], dtype=np.int64)
    sp = np.concatenate([[0], np.cumsum(ns)[:-1]]).astype(np.int64)
    lens = np.array([len(s) for s in seqs], dtype=np.int32)
    b = dict(reads=np.frombuffer(b"".join(seqs), dtype=np.uint8).copy(), read_len=lens,
             read_ptr=np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64))
    return b, np.concatenate(sigs).astype(np.float32), sp, ns, sc


def _table_words(v, j):
    """read j's malloc()ed table as the library wrote it, 6 uint32 per event_t, tail padding included (a numpy copy of a structured
    array does not copy padding bytes)"""
    ne = int(v["n_events"][j])
    if ne == 0 or not v["ev_pp"][j]:
        return np.zeros((0, 6), dtype=np.uint32)
    return np.ctypeslib.as_array(C.cast(int(v["ev_pp"][j]), C.POINTER(C.c_uint32)), shape=(ne * 6,)).reshape(-1, 6).copy()


def _same(a, b):
    """bit equality of two arrays field by field (structured arrays: padding is not part of any contract)"""
    if a.dtype.names is None:
        return a.shape == b.shape and a.tobytes() == b.tobytes()
    return a.shape == b.shape and all(np.ascontiguousarray(a[f]).tobytes() == np.ascontiguousarray(b[f]).tobytes() for f in a.dtype.names)


def _run(ctx, k, b, sig, sp, ns, sc, mode, ev_fields, rna=False):
    """one call; every output copied out of the view, the view freed"""
    v = ctx.signal_view(sig, sp, ns, sc, batch=b, want_pairs=(mode == "process"), rna=rna)
    (ctx.process_view if mode == "process" else ctx.events_view)(v, ev_fields=ev_fields)
    n = len(ns)
    o = dict(st=ctx.stats(), n_events=v["n_events"].copy(), ev=[ctx.view_events(v, j) for j in range(n)],
             words=[_table_words(v, j) for j in range(n)], scalings=v["scalings"].copy())
    if mode == "process":
        o.update(pairs=[ctx.view_pairs(v, j) for j in range(n)], n_pairs=v["n_pairs"].copy(), diag=v["diag"].copy(),
                 maps=[ctx.view_map(v, j, int(b["read_len"][j]) - k + 1) for j in range(n)],
                 scalings_estimated=v["scalings_estimated"].copy(), events_per_base=v["events_per_base"].copy(),
                 read_stat_flag=v["read_stat_flag"].copy(), n_event_alignment=v["n_event_alignment"].copy())
    ctx.free_view(v)
    return o


def _check_selection(o, ref, ev_fields, mode):
    """o: a run under ev_fields, ref: the ALL run of the same batch"""
    assert (o["n_events"] == ref["n_events"]).all()
    assert _same(o["scalings"], ref["scalings"])
    for j, (g, a) in enumerate(zip(o["ev"], ref["ev"])):
        assert len(g) == len(a), j
        for f in FIELDS[ev_fields]:
            assert _same(g[f], a[f]), (j, f)
        w = o["words"][j]
        for q in ZERO_WORDS[ev_fields]:
            assert (w[:, q] == 0).all(), (j, ev_fields, q)                  # +0.0f and zero padding, not just "== 0.0"
    if mode == "process":
        for key in ("n_pairs", "diag", "scalings_estimated", "events_per_base", "read_stat_flag", "n_event_alignment"):
            assert _same(o[key], ref[key]), key
        for j in range(len(o["pairs"])):
            assert _same(o["pairs"][j], ref["pairs"][j]), j
            assert (o["maps"][j] is None) == (ref["maps"][j] is None) and (o["maps"][j] is None or (o["maps"][j] == ref["maps"][j]).all()), j


def _check_oracle(orc, o, sig, sp, ns, sc, rna, reads):
    for j in reads:
        o_ev, _ = orc.getevents(sig[sp[j]:sp[j] + ns[j]].astype(np.int16), *[float(x) for x in sc[j]], rna=rna)
        if rna:
            o_ev = orc.reverse_events(o_ev)                                 # event_single writes RNA tables 3'->5' (f5c.c:711-719)
        g = o["ev"][j]
        assert len(g) == len(o_ev), j
        for f in ("start", "length", "mean", "stdv"):
            assert (g[f] == o_ev[f]).all(), (j, f)


@pytest.mark.gpu
@pytest.mark.parametrize("rna", [False, True], ids=["dna", "rna"])
@pytest.mark.parametrize("mode", ["events", "process"])
def test_selected_fields_equal_the_full_tables_and_nothing_else_changes(ctx, orc, r9, monkeypatch, mode, rna):
    from f5c_amd import abea
    _pipeline_env(monkeypatch)
    if rna:
        k, model = rna_model()
        b, sig, sp, ns, sc = _rna_batch(48, 4711)
        c = abea.AbeaContext(model, k, device_id=0, max_arena_bytes=4 << 30)
    else:
        k, model = r9
        b, sig, sp, ns, sc = _batch_and_signals(r9, 48, 31337, 1700)
        c = ctx
    try:
        runs = {s: _run(c, k, b, sig, sp, ns, sc, mode, s, rna=rna) for s in SELECTIONS}
        runs2 = {s: _run(c, k, b, sig, sp, ns, sc, mode, s, rna=rna) for s in reversed(SELECTIONS)}
    finally:
        if rna:
            c.close()
    ref = runs[ALL]
    assert ref["st"]["n_sub_batches"] >= 5
    _check_oracle(orc, ref, sig, sp, ns, sc, rna, range(48))
    for s in SELECTIONS:
        _check_selection(runs[s], ref, s, mode)
        _check_selection(runs2[s], ref, s, mode)
        for j in range(48):                                                 # repeatable whole-struct, padding included
            assert (runs[s]["words"][j] == runs2[s]["words"][j]).all(), (s, j)
    if mode == "process":
        assert int((ref["n_pairs"] > 0).sum()) >= 24
    # the tables are what comes down (event_db alone: per-read counts + scalings besides them)
    n_ev = int(ref["n_events"].sum())
    d2h = {s: runs[s]["st"]["d2h_bytes"] for s in SELECTIONS}
    assert d2h[LAYOUT] < d2h[NO_STDV] < d2h[ALL]
    for s in SELECTIONS:
        assert runs2[s]["st"]["d2h_bytes"] == d2h[s]
        if mode == "events":
            assert WIDTH[s] * n_ev <= d2h[s] <= WIDTH[s] * n_ev + 48 * 64 * 48, (s, d2h[s], n_ev)
        else:                                                               # same chunks, same result blocks: only the tables differ
            assert (WIDTH[ALL] - WIDTH[s]) * n_ev <= d2h[ALL] - d2h[s] <= (WIDTH[ALL] - WIDTH[s]) * n_ev + 48 * 48, s


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["events", "process"])
def test_overflowed_tables_follow_the_selection(ctx, orc, r9, monkeypatch, mode):
    """ABEA_CHAIN_CAP_DIV=48: nearly every table overflows its first guess and is redone after the pipeline, whole event_t from the
    device; what comes back must be the table of the selection, byte for byte the one of a run without overflow."""
    k, model = r9
    b, sig, sp, ns, sc = _batch_and_signals(r9, 48, 2024, 1700)
    _pipeline_env(monkeypatch)
    plain = {s: _run(ctx, k, b, sig, sp, ns, sc, mode, s) for s in (NO_STDV, LAYOUT)}
    monkeypatch.setenv("ABEA_CHAIN_CAP_DIV", "48")
    ref = _run(ctx, k, b, sig, sp, ns, sc, mode, ALL)                       # redone too: every other output of the redo path
    assert int((ref["n_events"] > ns // 48 + 16).sum()) >= 40               # nearly all redone
    _check_oracle(orc, ref, sig, sp, ns, sc, False, range(48))
    for s in (LAYOUT, NO_STDV):
        o = _run(ctx, k, b, sig, sp, ns, sc, mode, s)
        _check_selection(o, ref, s, mode)
        for j in range(48):                                                 # redone or not: the same table, padding included
            assert (o["words"][j] == plain[s]["words"][j]).all(), (s, j)


@pytest.mark.gpu
def test_layout_on_a_two_device_context(orc, r9, monkeypatch):
    """one GPU listed twice (as test_process_chain_on_a_two_device_context): each device context gets the selection"""
    from f5c_amd import abea
    k, model = r9
    b, sig, sp, ns, sc = _batch_and_signals(r9, 50, 777, 2000)
    monkeypatch.setenv("ABEA_CHAIN_SLOTS", "2")
    monkeypatch.setenv("ABEA_CHAIN_CHUNK_SAMPLES", str(500_000))
    monkeypatch.setenv("ABEA_CHAIN_CHUNK_READS", "4")
    with abea.AbeaContext(model, k, device_ids=[0, 0], max_arena_bytes=3 << 30) as c2:
        assert c2.device_count() == 2
        ref = _run(c2, k, b, sig, sp, ns, sc, "process", ALL)
        o = _run(c2, k, b, sig, sp, ns, sc, "process", LAYOUT)
        eref = _run(c2, k, b, sig, sp, ns, sc, "events", ALL)
        e = _run(c2, k, b, sig, sp, ns, sc, "events", LAYOUT)
    assert o["st"]["n_devices"] == 2 and o["st"]["n_sub_batches"] >= 4 and e["st"]["n_devices"] == 2
    _check_selection(o, ref, LAYOUT, "process")
    _check_selection(e, eref, LAYOUT, "events")
    _check_oracle(orc, ref, sig, sp, ns, sc, False, range(0, 50, 5))


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [3, 0xFFFFFFFF])
def test_unknown_selection_is_refused_before_any_work(ctx, r9, bad):
    from f5c_amd import abea
    k, model = r9
    b, sig, sp, ns, sc = _batch_and_signals(r9, 6, 5, 1500)
    sig0 = sig.copy()
    for mode in ("events", "process"):
        v = ctx.signal_view(sig, sp, ns, sc, batch=b, want_pairs=(mode == "process"), to_pa=True)
        v["ev_pp"][:] = 0xDEAD0000                                          # whatever the caller's array held: NULL afterwards
        with pytest.raises(abea.AbeaError, match="ev_fields"):
            (ctx.process_view if mode == "process" else ctx.events_view)(v, ev_fields=bad)
        assert (v["ev_pp"] == 0).all() and (v["n_events"] == 0).all()
        if mode == "process":
            assert (v["pairs_pp"] == 0).all() and (v["map_pp"] == 0).all()
        assert (sig == sig0).all()                                          # not even the pA conversion ran
    v = ctx.signal_view(sig, sp, ns, sc, batch=b)                           # the context is unharmed
    ctx.events_view(v, ev_fields=LAYOUT)
    assert (v["ev_pp"] != 0).all()
    ctx.free_view(v)


@pytest.mark.gpu
def test_read1_printed_table_through_both_entries(ctx, orc, r9):
    """The reference's printed table of test/ecoli_2kb_region's single read (7165 events from 36 121 samples)"""
    k, model = r9
    g = np.load(os.path.join(GOLD, "read1_events.npz"))
    sig = g["signal"].astype(np.float32)
    sp, ns, sc = np.array([0], np.int64), np.array([len(sig)], np.int64), g["scaling"].reshape(1, 3)
    seq = g["seq"].tobytes()
    b = dict(reads=g["seq"].copy(), read_len=np.array([len(seq)], np.int32), read_ptr=np.array([0], np.int64))
    for mode in ("events", "process"):
        runs = {s: _run(ctx, k, b, sig, sp, ns, sc, mode, s) for s in SELECTIONS}
        lay, full = runs[LAYOUT]["ev"][0], runs[ALL]["ev"][0]
        assert len(lay) == len(full) == 7165
        assert (lay["start"] == g["start"]).all() and (lay["length"] == g["length"]).all()
        assert [b"%.6f" % x for x in full["mean"]] == list(g["mean_txt"])
        assert [b"%.6f" % x for x in full["stdv"]] == list(g["stdv_txt"])
        for s in SELECTIONS:
            _check_selection(runs[s], runs[ALL], s, mode)
        if mode == "process":
            o_ev, _, (scale, shift), o_pairs, rec = _oracle_chain(orc, model, k, seq, g["signal"], g["scaling"])
            for s in SELECTIONS:
                o = runs[s]
                assert len(o_pairs) > 0 and _same(o["pairs"][0], o_pairs), s
                m = o["maps"][0]
                assert (m[:, 0] == rec["base_to_event_map"]["start"]).all() and (m[:, 1] == rec["base_to_event_map"]["stop"]).all()
                assert o["scalings_estimated"]["scale"][0] == np.float32(scale) and o["scalings_estimated"]["shift"][0] == np.float32(shift)
                assert int(o["read_stat_flag"][0]) == rec["flag"] and float(o["events_per_base"][0]) == rec["events_per_base"]
                for f in ("shift", "scale", "var", "log_var"):
                    assert o["scalings"][f][0] == rec["scalings"][f], (s, f)


@pytest.mark.gpu
def test_cpp_resquiggle_caller_prints_the_same_from_layout_tables(tmp_path, r9):
    """tests/fields_driver.cpp (plain g++, no Python in the chain): the 10 real reads of ecoli_reads.npz through
    abea_f5c_process_fields(LAYOUT) and abea_f5c_process; output_db_rsq's TSV and PAF are byte-identical while the first call
    brings down a third of the table bytes."""
    k, model = r9
    reads = _raw_reads()
    exe = str(tmp_path / "fields_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O2", os.path.join(ROOT, "tests", "fields_driver.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "f5c_amd"), "-labea_hip", "-Wl,-rpath," + os.path.join(ROOT, "f5c_amd")])
    _dump(str(tmp_path / "b.bin"), model, k, 0, reads)
    subprocess.check_call([exe, str(tmp_path / "b.bin"), str(tmp_path / "o")], env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    out = str(tmp_path / "o")
    for ext in (".tsv", ".paf", ".state"):
        assert open(out + ".layout" + ext, "rb").read() == open(out + ".all" + ext, "rb").read(), ext
    tsv, paf = open(out + ".all.tsv").read(), open(out + ".all.paf").read()
    assert tsv.count("\n") > 50000 and paf.count("\n") == 10
    ev_dt = np.dtype([("start", "<u8"), ("length", "<f4"), ("mean", "<f4"), ("stdv", "<f4")], align=True)
    tabs, words = {}, {}
    for s in ("layout", "all"):
        raw = open(out + "." + s + ".events", "rb").read()
        pos, t, w = 0, [], []
        for _ in range(len(reads)):
            ne = int(np.frombuffer(raw[pos:pos + 8], dtype=np.uint64)[0]); pos += 8
            t.append(np.frombuffer(raw[pos:pos + 24 * ne], dtype=ev_dt))
            w.append(np.frombuffer(raw[pos:pos + 24 * ne], dtype=np.uint32).reshape(-1, 6)); pos += 24 * ne
        tabs[s], words[s] = t, w
    for a, f, w in zip(tabs["layout"], tabs["all"], words["layout"]):
        assert len(a) == len(f) > 0
        assert (a["start"] == f["start"]).all() and (a["length"] == f["length"]).all()
        assert (w[:, 3:] == 0).all()                                        # mean, stdv, padding: zero bits
    d2h_layout, d2h_all, n_ev = (int(x) for x in open(out + ".bytes").read().split())
    assert n_ev == sum(len(t) for t in tabs["all"])
    assert 8 * n_ev <= d2h_all - d2h_layout <= 8 * n_ev + 48 * len(reads)   # 12 -> 4 bytes per event: a third of the table bytes
