"""CPU: the oracle's per-read chain (event detection -> scalings -> ABEA -> recalibration) against the
reference's goldens for test/ecoli_2kb_region (adaptive.exp, est_scalings.exp, recalib_scalings.exp)."""
import os
import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _reads():
    z = np.load(os.path.join(GOLD, "ecoli_reads.npz"))
    for i in range(int(z["n"])):
        off, rng, dig = z["scaling"][i]
        yield dict(sig=z[f"sig{i}"], seq=z[f"seq{i}"].tobytes(), offset=off, range=rng, digitisation=dig,
                   ada=str(z["ada"][i]), ada_printed=str(z["ada_printed"][i]), est=str(z["est"][i]), rec=str(z["rec"][i]), n_events=int(z["n_events"][i]),
                   read_id=str(z["read_id"][i]))


def test_real_signal_chain_matches_reference_goldens(orc, r9):
    """10 real reads (raw FAST5 signal committed as data): printed est_scalings / recalib_scalings lines equal
    the reference's, n_aligned_events exact, sum_emission to 1e-6 relative."""
    k, model = r9
    n = 0
    for r in _reads():
        ev, _ = orc.getevents(r["sig"], r["offset"], r["range"], r["digitisation"])
        assert len(ev) == r["n_events"]
        scale, shift = orc.estimate_scalings(r["seq"], model, k, ev)
        assert "%.2f %.2f" % (shift, scale) == r["est"]                 # est_scalings.exp
        pairs, d = orc.align(r["seq"], ev, model, k, scale, shift)
        gsum, gn = r["ada"].split()
        assert d["n_aligned"] == int(gn) == len(pairs)                   # the oracle's own record at fixture time
        assert abs(d["sum_emission"] - float(gsum)) <= 1e-6
        psum, pn = r["ada_printed"].split()                              # adaptive.exp as the reference printed it
        assert d["n_aligned"] == int(pn)
        assert abs(d["sum_emission"] - float(psum)) <= 1e-6 * abs(float(psum)) + 1e-6
        rec = orc.scaling_single(pairs, r["seq"], ev, model, k, scale, shift)
        assert "%.2f %.2f %.2f" % (rec["scalings"]["shift"], rec["scalings"]["scale"], rec["scalings"]["var"]) == r["rec"]
        n += 1
    assert n == 10


# Every FAST5 of the test set (112 reads, 5.5 M raw samples: more than a fixture here should hold) through the same chain is
# tests/golden/make_ecoli_golden.py --check, run where the f5c test data is; the committed fixtures cover 10 reads from the raw
# signal (above) and all 111 reads of the BAM from their event tables (test_all_111_reads_mean_only_events_against_printed_goldens below).


@pytest.mark.gpu
def test_gpu_bit_exact_on_real_signal_reads(ctx, orc, r9):
    """HIP path on real nanopore reads (events from the oracle's event detection) vs the oracle."""
    from f5c_amd import synth
    k, model = r9
    seqs, evs, scs = [], [], []
    for r in _reads():
        ev, _ = orc.getevents(r["sig"], r["offset"], r["range"], r["digitisation"])
        scale, shift = orc.estimate_scalings(r["seq"], model, k, ev)
        seqs.append(r["seq"]); evs.append(ev); scs.append((scale, shift))
    batch = synth.batch_from_reads(seqs, evs, scs)
    d = ctx.upload(batch)
    ctx.align_db_device(d)
    pairs, n_pairs, diag = ctx.download(d)
    o_pairs, o_n, o_diag = orc.align_batch(batch, model, k, n_threads=8)
    assert (n_pairs == o_n).all() and (o_n > 0).all()
    for i in range(len(o_n)):
        s = int(batch["pair_ptr"][i])
        assert (pairs[s:s + o_n[i]] == o_pairs[s:s + o_n[i]]).all()
    assert np.allclose(diag["sum_emission"], o_diag["sum_emission"], rtol=0, atol=1e-4)


@pytest.mark.gpu
def test_gpu_event_detection_bit_exact(ctx, orc, r9):
    """Row N2: raw ADC signal -> events + method-of-moments scalings on the device, bit-exact against the oracle's
    event detection (itself pinned to est_scalings.exp / adaptive.exp), on real reads and synthetic signals."""
    from f5c_amd import synth
    k, model = r9
    reads = list(_reads())
    sigs = [r["sig"] for r in reads]
    scal = np.array([[r["offset"], r["range"], r["digitisation"]] for r in reads], dtype=np.float32)
    seqs = [r["seq"] for r in reads]
    b = synth.make_batch(40, model, k, seed=91, law=1500, bad_frac=0.0)
    s_sigs, s_scal = synth.make_signals(b, seed=3)
    for i in range(40):
        s, L = int(b["read_ptr"][i]), int(b["read_len"][i])
        seqs.append(b["reads"][s:s + L].tobytes())
    sigs += s_sigs
    scal = np.concatenate([scal, s_scal])
    evs, ne, sc = ctx.detect_events_device(sigs, scal, seqs=seqs)
    for i, sig in enumerate(sigs):
        o_ev, _ = orc.getevents(sig, scal[i, 0], scal[i, 1], scal[i, 2])
        assert ne[i] == len(o_ev), (i, ne[i], len(o_ev))
        for f in ("start", "length", "mean", "stdv"):
            assert (evs[i][f] == o_ev[f]).all(), (i, f)
        scale, shift = orc.estimate_scalings(seqs[i], model, k, o_ev)
        assert sc["scale"][i] == np.float32(scale) and sc["shift"][i] == np.float32(shift)
    # the printed est_scalings.exp lines of the real reads come out of the device path too
    for i, r in enumerate(reads):
        assert "%.2f %.2f" % (sc["shift"][i], sc["scale"][i]) == r["est"]
    assert 5 < np.mean([len(s) / max(1, n) for s, n in zip(sigs, ne)]) < 15     # ~10 samples per event


@pytest.mark.gpu
def test_gpu_event_detection_adversarial_signals(ctx, orc):
    """The segment-parallel detector must equal the sequential one on signals where speculative segments do not
    re-synchronise quickly (plateaus, pure noise, slow waves: these take the per-read sequential fallback) and on
    degenerate lengths."""
    r = np.random.default_rng(5)
    sigs = [np.full(5000, 500, np.int16), np.full(7, 500, np.int16), np.full(1, 500, np.int16),
            np.full(513, 480, np.int16), np.arange(400, 1424, dtype=np.int16),
            r.integers(300, 700, 100000).astype(np.int16),
            np.repeat(r.integers(300, 700, 400), 250).astype(np.int16),
            (np.repeat(r.integers(300, 700, 30000), 3) + r.integers(-2, 3, 90000)).astype(np.int16),
            (500 + 100 * np.sin(np.arange(200000) / 50.0)).astype(np.int16),
            (500 + 60 * np.sin(np.arange(70000) / 700.0) + r.normal(0, 0.6, 70000)).astype(np.int16)]
    scal = np.tile(np.array([10.0, 1467.61, 8192.0], dtype=np.float32), (len(sigs), 1))
    # a channel offset that puts some samples within 1e-3 pA of zero: the prefix sums are then not provably exact in
    # every order and that read must take the sequential sums kernel
    sigs.append(r.integers(495, 700, 60000).astype(np.int16))
    scal = np.concatenate([scal, np.array([[-499.999, 1467.61, 8192.0]], dtype=np.float32)])
    evs, ne, _ = ctx.detect_events_device(sigs, scal, cap_div=1)
    for i, sig in enumerate(sigs):
        o_ev, _ = orc.getevents(sig, scal[i, 0], scal[i, 1], scal[i, 2])
        assert ne[i] == len(o_ev), (i, ne[i], len(o_ev))
        for f in ("start", "length", "mean", "stdv"):
            assert (evs[i][f] == o_ev[f]).all(), (i, f)


@pytest.mark.gpu
@pytest.mark.parametrize("rna", [False, True])
def test_gpu_detector_common_path_equals_the_array_and_sequential_forms(ctx, r9, monkeypatch, rna):
    """Round 6: the common path takes window and event sums straight from the samples (abea_ev_spec2 / fix2 / create2 kernels, no
    prefix-sum or t-statistic arrays) and hands flagged reads — sums that may round, segments that never meet their replay — to the
    array kernels behind it.  Its tables and scalings must equal, byte for byte, the array form of rounds 3-5 (ABEA_EV_PATH=arrays)
    and the fully sequential form (ABEA_EV_SEQUENTIAL), on real reads, synthetic reads, signals that take either fallback, reads
    shorter than a window and reads ending one sample into a segment."""
    from f5c_amd import synth
    k, model = r9
    r = np.random.default_rng(17)
    reads = list(_reads())
    sigs = [x["sig"] for x in reads]
    scal = [[x["offset"], x["range"], x["digitisation"]] for x in reads]
    seqs = [x["seq"] for x in reads]
    b = synth.make_batch(70, model, k, seed=92, law=3000, bad_frac=0.0)
    s_sigs, s_scal = synth.make_signals(b, seed=4)
    sigs += s_sigs; scal += [list(x) for x in s_scal]
    seqs += [b["reads"][int(b["read_ptr"][i]):int(b["read_ptr"][i]) + int(b["read_len"][i])].tobytes() for i in range(70)]
    extra = [np.full(5000, 500, np.int16), np.full(1, 500, np.int16), np.full(2, 300, np.int16), np.full(13, 500, np.int16),
             r.integers(300, 700, 512).astype(np.int16), r.integers(300, 700, 513).astype(np.int16),
             r.integers(300, 700, 1025).astype(np.int16), r.integers(300, 700, 100000).astype(np.int16),
             np.repeat(r.integers(300, 700, 400), 250).astype(np.int16),
             (500 + 100 * np.sin(np.arange(200000) / 50.0)).astype(np.int16),
             r.integers(-32768, 32767, 30000).astype(np.int16)]
    sigs += extra; scal += [[10.0, 1467.61, 8192.0]] * len(extra)
    sigs.append(r.integers(495, 700, 60000).astype(np.int16)); scal.append([-499.999, 1467.61, 8192.0])   # samples next to 0 pA: sums may round
    sigs.append(np.zeros(3000, np.int16)); scal.append([0.0, 1467.61, 8192.0])                               # all samples exactly 0 pA
    seqs += [bytes(r.choice(list(b"ACGT"), 700).astype(np.uint8))] * (len(extra) + 2)
    scal = np.array(scal, dtype=np.float32)

    def run(pad_to=8, **env):
        for name in ("ABEA_EV_PATH", "ABEA_EV_SEQUENTIAL"):
            monkeypatch.delenv(name, raising=False)
        for name, v in env.items():
            monkeypatch.setenv(name, v)
        return ctx.detect_events_device(sigs, scal, seqs=seqs, rna=rna, cap_div=1, pad_to=pad_to)
    evs, ne, sc = run()
    # pad_to=1: the signals packed back to back, i.e. reads starting at every 2-byte alignment (the staging rows of the common
    # path are filled from the 16-byte boundary below a lane's first sample, whatever that is)
    for form in (dict(ABEA_EV_PATH="arrays"), dict(ABEA_EV_SEQUENTIAL="1"), dict(pad_to=1), dict(pad_to=1, ABEA_EV_PATH="arrays")):
        evs2, ne2, sc2 = run(**form)
        assert (ne == ne2).all(), form
        for i in range(len(sigs)):
            for f in ("start", "length", "mean", "stdv"):                # field by field: event_t has 4 bytes of tail padding
                a, b2 = evs[i][f], evs2[i][f]
                assert a.tobytes() == b2.tobytes(), (form, i, f, len(sigs[i]))
        for f in ("scale", "shift"):
            assert (sc[f].view(np.uint32) == sc2[f].view(np.uint32)).all(), (form, f)
    assert ne.sum() > 100000


@pytest.mark.gpu
def test_gpu_raw_signal_to_recalibrated_scalings(ctx, orc, r9):
    """Whole device chain on real reads: raw signal -> events -> scalings -> ABEA -> scaling_single; the printed
    recalib_scalings.exp / adaptive.exp values of the reference come out of the GPU."""
    from f5c_amd import synth
    k, model = r9
    reads = list(_reads())
    # the event tables stay in HBM between the two calls (only n_events and the estimated scalings come to the host)
    d = ctx.signals_to_device_batch([r["sig"] for r in reads],
                                    np.array([[r["offset"], r["range"], r["digitisation"]] for r in reads]),
                                    [r["seq"] for r in reads])
    ctx.align_db_device(d, scaling=True)
    _, n_pairs, diag = ctx.download(d)
    _, rsc, _, flags, _ = ctx.download_scaling(d)
    for i, r in enumerate(reads):
        gsum, gn = r["ada_printed"].split()                              # GPU vs the reference's printed adaptive.exp record
        assert n_pairs[i] == int(gn)
        assert abs(diag["sum_emission"][i] - float(gsum)) <= 1e-6 * abs(float(gsum)) + 1e-6
        assert "%.2f %.2f %.2f" % (rsc["shift"][i], rsc["scale"][i], rsc["var"][i]) == r["rec"]
        assert flags[i] == 0


# ---- configs[0] on all 111 reads of the BAM: mean-only event tables (tests/golden/ecoli_events.npz) -------------------
def _all_reads():
    from f5c_amd.types import EVENT_DT
    z = np.load(os.path.join(GOLD, "ecoli_events.npz"))
    out = []
    for i in range(len(z["read_id"])):
        a, b = int(z["ev_ptr"][i]), int(z["ev_ptr"][i + 1])
        ev = np.zeros(b - a, dtype=EVENT_DT)
        ev["mean"] = z["mean"][a:b]                              # the only field ABEA / scaling_single read (align.c:131,738)
        s0, s1 = int(z["seq_ptr"][i]), int(z["seq_ptr"][i + 1])
        out.append(dict(read_id=str(z["read_id"][i]), seq=z["seq"][s0:s1].tobytes(), events=ev,
                        scale=np.float32(z["scale"][i]), shift=np.float32(z["shift"][i]),
                        printed_sum=float(z["printed_sum"][i]), printed_n=int(z["printed_n"][i]),
                        printed_avg=float(z["printed_avg"][i]), est=str(z["est"][i]), rec=str(z["rec"][i])))
    return out


def _check_vs_printed(r, n_aligned, sum_emission, rec_line):
    assert n_aligned == r["printed_n"], r["read_id"]                                        # adaptive.exp, exact
    assert abs(sum_emission - r["printed_sum"]) <= 1e-6 * abs(r["printed_sum"]) + 1e-6      # printed by a build whose sums differ in the 7th digit
    assert abs(sum_emission / n_aligned - r["printed_avg"]) < 5e-6
    assert "%.2f %.2f" % (r["shift"], r["scale"]) == r["est"]                               # est_scalings.exp
    if r["rec"]:                                                                            # recalib_scalings.exp (110 of 111 lines; read 95ff70e7 is the known odd one)
        assert rec_line == r["rec"], (r["read_id"], rec_line, r["rec"])


def test_all_111_reads_mean_only_events_against_printed_goldens(orc, r9):
    """Every read of the reference's BAM: oracle ABEA + scaling_single on the committed mean-only event tables against the
    reference's PRINTED adaptive.exp / recalib_scalings.exp records."""
    k, model = r9
    reads = _all_reads()
    assert len(reads) == 111
    n_rec = 0
    for r in reads:
        pairs, d = orc.align(r["seq"], r["events"], model, k, r["scale"], r["shift"])
        rec = orc.scaling_single(pairs, r["seq"], r["events"], model, k, r["scale"], r["shift"])
        sc = rec["scalings"]
        _check_vs_printed(r, int(d["n_aligned"]), float(d["sum_emission"]),
                          "%.2f %.2f %.2f" % (sc["shift"], sc["scale"], sc["var"]))
        n_rec += bool(r["rec"])
    assert n_rec >= 110


@pytest.mark.gpu
def test_gpu_all_111_reads_against_printed_goldens(ctx, orc, r9):
    """configs[0], GPU-vs-REFERENCE on all 111 reads: n_aligned_events equal to adaptive.exp, sum_emission to the
    fixture's 1e-6, recalibrated scalings equal to the printed recalib_scalings.exp lines; and GPU-vs-oracle bit-exact
    pair lists, through the device entry and the host entry."""
    from f5c_amd import synth
    k, model = r9
    reads = _all_reads()
    batch = synth.batch_from_reads([r["seq"] for r in reads], [r["events"] for r in reads],
                                   [(r["scale"], r["shift"]) for r in reads])
    d = ctx.upload(batch)
    ctx.align_db_device(d, scaling=True)
    pairs, n_pairs, diag = ctx.download(d)
    _, rsc, _, flags, _ = ctx.download_scaling(d)
    for i, r in enumerate(reads):
        _check_vs_printed(r, int(n_pairs[i]), float(diag["sum_emission"][i]),
                          "%.2f %.2f %.2f" % (rsc["shift"][i], rsc["scale"][i], rsc["var"][i]))
    o_pairs, o_n, o_diag = orc.align_batch(batch, model, k, n_threads=8)
    assert (n_pairs == o_n).all()
    h_pairs, h_n, _ = ctx.align_flat_host(batch)
    assert (h_n == o_n).all()
    for i in range(len(o_n)):
        s = int(batch["pair_ptr"][i])
        assert (pairs[s:s + o_n[i]] == o_pairs[s:s + o_n[i]]).all()
        assert (h_pairs[i] == o_pairs[s:s + o_n[i]]).all()
    assert (diag["sum_emission"] == o_diag["sum_emission"]).all()
