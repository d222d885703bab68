#!/usr/bin/env python3
"""Mint tests/golden/read1_events.npz: the reference's printed event table of test/ecoli_2kb_region's single read, with its raw signal.

single_read/read1.events.exp prints all 7165 events of read fa9ad683-35c5-4dad-a3af-de7a86b1ffa8 as
{start,length,mean,stdv,-1,-1}, floats to 6 decimals; the read's raw signal is fast5_files/..._ch85_read2098_strand.fast5.
Run in the build container only (needs the reference's test data and h5dump, as make_ecoli_golden.py).  Reads DATA files only:
the FAST5 (int16 signal + channel scaling), read1.fasta (the sequence) and read1.events.exp.  Writes the signal, offset / range /
digitisation, the sequence, start and length as numbers and the printed text of mean and stdv, so that a test compares "%.6f"
strings (tests/test_read1_events_pin.py, tests/test_event_fields.py).  --check: verify the oracle reproduces the table, write nothing.
"""
import glob
import os
import re
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_ecoli_golden import REF, ROOT, read_fast5  # noqa: E402

READ_ID = "fa9ad683-35c5-4dad-a3af-de7a86b1ffa8"


def parse_events(path):
    rows = re.findall(r"\{(\d+),([-0-9.]+),([-0-9.]+),([-0-9.]+),-1,-1\}", open(path).read())
    start = np.array([int(r[0]) for r in rows], dtype=np.uint64)
    length = np.array([float(r[1]) for r in rows], dtype=np.float32)
    return start, length, np.array([r[2] for r in rows], dtype="S16"), np.array([r[3] for r in rows], dtype="S16")


def main(write=True):
    (f5path,) = glob.glob(os.path.join(REF, "fast5_files", "*_ch85_read2098_strand.fast5"))
    f5 = read_fast5(f5path)
    assert f5["read_id"] == READ_ID, f5["read_id"]
    seq = "".join(l.strip() for l in open(os.path.join(REF, "single_read", "read1.fasta")) if not l.startswith(">")).encode()
    start, length, mean_txt, stdv_txt = parse_events(os.path.join(REF, "single_read", "read1.events.exp"))
    assert len(start) == 7165 and len(f5["signal"]) == 36121
    sys.path.insert(0, ROOT)
    from oracle import orc
    ev, _ = orc.getevents(f5["signal"], f5["offset"], f5["range"], f5["digitisation"])
    assert len(ev) == len(start) and (ev["start"] == start).all() and (ev["length"] == length).all()
    assert [b"%.6f" % x for x in ev["mean"]] == list(mean_txt) and [b"%.6f" % x for x in ev["stdv"]] == list(stdv_txt)
    print(f"oracle getevents reproduces all {len(start)} printed events of {READ_ID}")
    if write:
        np.savez_compressed(os.path.join(HERE, "read1_events.npz"), read_id=np.array(READ_ID), signal=f5["signal"].astype(np.int16),
                            scaling=np.array([f5["offset"], f5["range"], f5["digitisation"]], dtype=np.float32),
                            seq=np.frombuffer(seq, dtype=np.uint8), start=start, length=length, mean_txt=mean_txt, stdv_txt=stdv_txt)


if __name__ == "__main__":
    sys.exit(main(write="--check" not in sys.argv))
