#!/usr/bin/env python3
"""Mint tests/golden/meth_golden.npz: what call-methylation (mode 0) needs of test/ecoli_2kb_region that is not an event table.

Data only, from the reference's test files; no htslib, no network.  A pure-Python BGZF/BAM reader (gzip + struct) takes from
single_read/read1.sorted.bam and reads.sorted.bam every record's read name, flag, mapq, contig, pos and CIGAR words.  The printed
outputs give the reference windows that are known: the m_seq window of each of single_read/meth_input.exp's 45 CpG groups (it
starts 10 bases before the group's first CpG, meth.c:518) and the `sequence` column of single_read/meth.exp and meth.exp (it
starts k-1 bases before the first CpG, meth.c:591), with their absolute positions.  draft.fa is not in the reference tree, so
tests build a synthetic segment from these windows over a filler of 'A' (tests/meth_restate.py: synthetic_segment).

Run where the reference's test data is (make_ecoli_golden.REF); --check verifies and writes nothing."""
import gzip
import os
import re
import struct
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_ecoli_golden import REF  # noqa: E402  the reference's test/ecoli_2kb_region
K = 6


def read_bam(path):
    """Every alignment record of a BAM file: dict(name, flag, mapq, tid, pos, cigar (uint32 words), l_seq)."""
    raw = gzip.decompress(open(path, "rb").read())          # BGZF = concatenated gzip members
    assert raw[:4] == b"BAM\1", path
    o = 4
    (l_text,) = struct.unpack_from("<i", raw, o); o += 4 + l_text
    (n_ref,) = struct.unpack_from("<i", raw, o); o += 4
    contigs = []
    for _ in range(n_ref):
        (l_name,) = struct.unpack_from("<i", raw, o); o += 4
        contigs.append(raw[o:o + l_name - 1].decode()); o += l_name
        o += 4                                              # l_ref
    recs = []
    while o < len(raw):
        (block,) = struct.unpack_from("<i", raw, o)
        tid, pos, l_name, mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHi", raw, o + 4)
        p = o + 36
        name = raw[p:p + l_name - 1].decode(); p += l_name
        cigar = np.frombuffer(raw[p:p + 4 * n_cig], dtype="<u4").astype(np.uint32)
        recs.append(dict(name=name, flag=flag, mapq=mapq, tid=tid, pos=pos, cigar=cigar, l_seq=l_seq))
        o += 4 + block
    return contigs, recs


def ref_span(cigar):
    """bam_endpos - pos: M, D, N, =, X consume the reference"""
    return int(sum(int(w) >> 4 for w in cigar if (int(w) & 15) in (0, 2, 3, 7, 8)))


def meth_rows(path, header):
    rows = [l.rstrip("\n").split("\t") for l in open(path)]
    if header:
        rows = rows[1:]
    return rows


def main(write=True):
    out = {}
    for tag, bam in (("read1", os.path.join(REF, "single_read", "read1.sorted.bam")), ("ecoli", os.path.join(REF, "reads.sorted.bam"))):
        contigs, recs = read_bam(bam)
        out[tag + "_contigs"] = np.array(contigs)
        out[tag + "_name"] = np.array([r["name"] for r in recs])
        out[tag + "_flag"] = np.array([r["flag"] for r in recs], dtype=np.int32)
        out[tag + "_mapq"] = np.array([r["mapq"] for r in recs], dtype=np.int32)
        out[tag + "_tid"] = np.array([r["tid"] for r in recs], dtype=np.int32)
        out[tag + "_pos"] = np.array([r["pos"] for r in recs], dtype=np.int32)
        out[tag + "_l_seq"] = np.array([r["l_seq"] for r in recs], dtype=np.int32)
        out[tag + "_cigar_ptr"] = np.cumsum([0] + [len(r["cigar"]) for r in recs]).astype(np.int64)
        out[tag + "_cigar"] = np.concatenate([r["cigar"] for r in recs]).astype(np.uint32)
        print(f"{bam}: {len(recs)} records on {contigs}")
    # single read: the 90 m_seq windows (two per group, the unmethylated one first) and the 45 printed rows
    txt = open(os.path.join(REF, "single_read", "meth_input.exp")).read()
    m_seq = re.findall(r"m_seq : (\S+)", txt)[0::2]
    rows = meth_rows(os.path.join(REF, "single_read", "meth.exp"), header=True)
    assert len(m_seq) == len(rows) == 45
    out["read1_meth_exp"] = np.array(open(os.path.join(REF, "single_read", "meth.exp")).read())   # the printed text, header included
    out["read1_win_seq"] = np.array(m_seq)
    out["read1_win_pos"] = np.array([int(r[1]) - 10 for r in rows], dtype=np.int32)       # sub_start_pos + ref_start_pos
    for s, r in zip(m_seq, rows):                                                          # the printed column lies inside the window
        assert s[10 - K + 1:10 - K + 1 + len(r[9])] == r[9], (s, r)
    # all reads: the printed `sequence` column of meth.exp with its absolute start (start - k + 1), one per row
    rows = meth_rows(os.path.join(REF, "meth.exp"), header=False)
    assert len(rows) == 20630
    out["ecoli_row_read"] = np.array([r[3] for r in rows])
    out["ecoli_row_contig"] = np.array([r[0] for r in rows])
    out["ecoli_row_start"] = np.array([int(r[1]) for r in rows], dtype=np.int32)
    out["ecoli_row_end"] = np.array([int(r[2]) for r in rows], dtype=np.int32)
    out["ecoli_row_ncpg"] = np.array([int(r[8]) for r in rows], dtype=np.int32)
    out["ecoli_row_seq"] = np.array([r[9] for r in rows])
    if write:
        np.savez_compressed(os.path.join(HERE, "meth_golden.npz"), **out)
        print("wrote meth_golden.npz")


if __name__ == "__main__":
    sys.exit(main(write="--check" not in sys.argv))
