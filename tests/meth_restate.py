"""Test support: a Python restatement of calculate_methylation_for_read (reference src/meth.c:473-612) for one read, scoring through
the oracle's profile_hmm_score (oracle/orc.py).  Serial and literal, so that tests can pin the GPU entry abea_meth_batch_host to it.

Kept as the reference behaves: get_next_event never visits its `stop` index; the record is dropped when its first and last event
are equal; the ratio test divides by calling_start - calling_end (negative), so it never rejects; right_bounded is always true
after a lower bound; sites come out ordered by start_position with strands_scored = 1.  The one divergence of the library is
restated too: a group whose bound is -1 or outside the event table, or whose stride does not match the strand (the reference
passes (uint32_t)-1 into the HMM or asserts), is skipped and counted."""
import numpy as np

IUPAC_FIRST = {"A": "A", "C": "C", "G": "G", "T": "T", "M": "A", "R": "A", "W": "A", "S": "C", "Y": "C", "K": "G", "V": "A",
               "H": "A", "D": "A", "B": "C", "N": "A"}
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
BAM_OPS = "MIDNSHP=X"


def disambiguate(seg: str) -> str:
    return "".join(IUPAC_FIRST[c] for c in seg.upper())


def methylate(s: str) -> str:
    return "".join("M" if s[i] == "C" and i + 1 < len(s) and s[i + 1] == "G" else s[i] for i in range(len(s)))


def reverse_complement(s: str) -> str:
    return "".join(COMP[c] for c in reversed(s))


def reverse_complement_meth(m: str) -> str:
    out = []
    i = 0
    while i < len(m):
        if m[i] == "M" and i + 1 < len(m) and m[i + 1] == "G":
            out += ["G", "M"]
            i += 2
        else:
            out.append(COMP[m[i]])
            i += 1
    return "".join(reversed(out))


def event_alignment_record(pos, cigar, rc, read_len, b2e_start, k):
    """get_event_alignment_record (meth.c:127-185): [(ref_pos, event_idx)]; None for an N or unknown CIGAR op"""
    seg = []
    read_pos, ref_pos = 0, pos
    for w in cigar:
        n, op = int(w) >> 4, int(w) & 15
        if op in (0, 7, 8):
            seg += [(ref_pos + j, read_pos + j) for j in range(n)]
            read_pos += n; ref_pos += n
        elif op == 2:
            ref_pos += n
        elif op in (1, 4):
            read_pos += n
        elif op == 5:
            pass
        else:
            return None
    map_size = read_len - k + 1

    def next_event(start, stop, stride):
        while start != stop:
            if b2e_start[start] != -1:
                return int(b2e_start[start])
            start += stride
        return -1

    out = []
    for ref, rp in seg:
        if rp < k or rp + k >= read_len:
            continue
        kidx = read_len - rp - k if rc else rp
        before = next_event(kidx, max(0, kidx - 1000), -1)
        after = next_event(kidx, min(kidx + 1000, map_size - 1), 1)
        out.append((ref, after if before == -1 else before))
    if out and out[0][1] == out[-1][1]:
        out = []
    return out


def event_alignment_record_np(pos, cigar, rc, read_len, b2e_start, k):
    """event_alignment_record with numpy: the same list, found through the nearest mapped k-mer at or before / at or after each
    position instead of a walk (the walk visits kidx .. stop_before + 1 and kidx .. stop_after - 1)"""
    ops = [(int(w) >> 4, int(w) & 15) for w in cigar]
    if any(op not in (0, 1, 2, 4, 5, 7, 8) for _, op in ops):
        return None
    ref_l, read_l = [], []
    read_pos, ref_pos = 0, pos
    for n, op in ops:
        if op in (0, 7, 8):
            ref_l.append(np.arange(ref_pos, ref_pos + n)); read_l.append(np.arange(read_pos, read_pos + n))
        read_pos += n if op in (0, 1, 4, 7, 8) else 0
        ref_pos += n if op in (0, 2, 7, 8) else 0
    if not ref_l:
        return []
    ref, rp = np.concatenate(ref_l), np.concatenate(read_l)
    keep = (rp >= k) & (rp + k < read_len)
    ref, rp = ref[keep], rp[keep]
    if not len(rp):
        return []
    m = np.asarray(b2e_start, dtype=np.int64)
    map_size = read_len - k + 1
    idx = np.arange(map_size)
    prev = np.maximum.accumulate(np.where(m != -1, idx, -1))
    nxt = np.minimum.accumulate(np.where(m != -1, idx, map_size)[::-1])[::-1]
    kidx = read_len - rp - k if rc else rp
    pb = prev[kidx]
    before = np.where(pb > np.maximum(0, kidx - 1000), m[np.maximum(pb, 0)], -1)
    na = nxt[kidx]
    after = np.where(na < np.minimum(kidx + 1000, map_size - 1), m[np.minimum(na, map_size - 1)], -1)
    ev = np.where(before == -1, after, before)
    if ev[0] == ev[-1]:
        return []
    return list(zip(ref.tolist(), ev.tolist()))


def lower_bound(rec, v):
    lo, hi = 0, len(rec)
    while lo < hi:
        mid = lo + (hi - lo) // 2
        if rec[mid][0] < v:
            lo = mid + 1
        else:
            hi = mid
    return lo


def plan_read(segment: str, pos, cigar, rc, read_len, b2e_start, n_events, k, fast=False):
    """The groups calculate_methylation_for_read scores: list of dict(start, end, n_cpg, e1, e2, stride, seq_u, seq_m) where
    seq_u / seq_m are the sequences the HMM reads (the reverse complements on a reverse read), and the number of groups skipped
    for a bound of -1 or outside the table.  None when the CIGAR holds an N or an unknown op."""
    ref = disambiguate(segment)
    rec = (event_alignment_record_np if fast else event_alignment_record)(pos, cigar, rc, read_len, b2e_start, k)
    if rec is None:
        return None, 0
    cpg = [i for i in range(len(ref) - 1) if ref[i] == "C" and ref[i + 1] == "G"]
    groups, cur = [], 0
    while cur < len(cpg):
        end = cur + 1
        while end < len(cpg) and cpg[end] - cpg[end - 1] <= 10:
            end += 1
        groups.append((cur, end)); cur = end
    out, skipped = [], 0
    for a, b in groups:
        sub_start, sub_end, span = cpg[a] - 10, cpg[b - 1] + 10, cpg[b - 1] - cpg[a]
        if sub_start <= 10 or span > 200:
            continue
        subseq = ref[sub_start:sub_end + 1]
        cs, ce = sub_start + pos, sub_end + pos
        si, ti = lower_bound(rec, cs), lower_bound(rec, ce)
        if si == len(rec) or ti == len(rec):
            continue
        if not (rec[si][0] <= cs or si != 0):
            continue
        e1, e2 = rec[si][1], rec[ti][1]
        if abs(e2 - e1) <= 10:          # the ratio test (meth.c:547) divides by a negative number: never rejects
            continue
        stride = 1 if e1 <= e2 else -1
        if e1 < 0 or e2 < 0 or e1 >= n_events or e2 >= n_events or (stride == -1) != bool(rc):
            skipped += 1
            continue
        m = methylate(subseq)
        out.append(dict(start=cpg[a] + pos, end=cpg[b - 1] + pos, n_cpg=b - a, e1=e1, e2=e2, stride=stride,
                        m_seq=subseq, m_rc_seq=reverse_complement(subseq), mm_seq=m, mm_rc_seq=reverse_complement_meth(m)))
    return out, skipped


def score_read(orc, groups, events, scaling, cpgmodel, k, rc, events_per_base):
    """(ll_methylated, ll_unmethylated) float32 per group through the oracle (meth.c:562-570, hmm_flags = 3)"""
    ev = np.ascontiguousarray(events)
    res = []
    for g in groups:
        u = orc.profile_hmm_score(g["m_seq"].encode(), g["m_rc_seq"].encode(), ev, scaling, cpgmodel, k, g["e1"], g["e2"],
                                  g["stride"], rc, events_per_base, 3)
        m = orc.profile_hmm_score(g["mm_seq"].encode(), g["mm_rc_seq"].encode(), ev, scaling, cpgmodel, k, g["e1"], g["e2"],
                                  g["stride"], rc, events_per_base, 3)
        res.append((np.float32(m), np.float32(u)))
    return res


def synthetic_segment(length, windows, filler="A"):
    """A segment of `length` filler bases with each (relative offset, text) window written in"""
    s = bytearray(filler.encode() * length)
    for off, w in windows:
        off = int(off)
        lo = max(off, 0)
        s[lo:off + len(w)] = w[lo - off:min(len(w), length - off)].encode()
    return bytes(s[:length]).decode()


def ref_span(cigar):
    return int(sum(int(w) >> 4 for w in cigar if (int(w) & 15) in (0, 2, 3, 7, 8)))


def format_rows(contig, read_name, rc, segment, pos, sites, k, version=1, clip_start=-1, clip_end=-1):
    """output_db's lines for one read (f5c.c:1033-1062), sites = [(start, end, n_cpg, ll_m, ll_u)]"""
    ref = disambiguate(segment)
    lines = []
    for st, en, n, llm, llu in sites:
        if (clip_start != -1 and st < clip_start) or (clip_end != -1 and en >= clip_end):
            continue
        m, u = float(llm), float(llu)
        seq = ref[st - pos - k + 1:en - pos + k]
        head = f"{contig}\t{st}\t{en}\t" if version == 1 else f"{contig}\t{'-' if rc else '+'}\t{st}\t{en}\t"
        lines.append(head + f"{read_name}\t{m - u:.2f}\t{m:.2f}\t{u:.2f}\t1\t{n}\t{seq}\n")
    return "".join(lines)


HEADER = {1: "chromosome\tstart\tend\tread_name\tlog_lik_ratio\tlog_lik_methylated\tlog_lik_unmethylated\t"
             "num_calling_strands\tnum_cpgs\tsequence\n",
          2: "chromosome\tstrand\tstart\tend\tread_name\tlog_lik_ratio\tlog_lik_methylated\tlog_lik_unmethylated\t"
             "num_calling_strands\tnum_motifs\tsequence\n"}
