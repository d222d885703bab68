/* abea_meth.hip — the job builder of call-methylation (mode 0) on gfx950: what calculate_methylation_for_read does before its
 * profile_hmm_score calls (reference src/meth.c:473-612).  The jobs are then scored by abea_hmm_forward_kernel (abea_hmm.hip),
 * unchanged.
 *
 * Mapping: one wavefront per read; every step is a wave-wide scan, ballot or prefix over the read, none a lane-0 loop:
 *   1. the event-alignment record, built ONCE per read (the reference rebuilds it per group, meth.c:537): the CIGAR is read 64
 *      ops at a time, inclusive scans give every op its read / reference start (get_aligned_segments, meth.c:23-98: M/=/X aligned,
 *      D moves ref, I moves read, S moves read by 1, H nothing); the positions the boundary test keeps (meth.c:150-156) form one
 *      interval per aligned op, so a third scan gives every kept position its slot, and lanes take 64 slots at a time, each
 *      finding its op by a 6-step binary search over the scan (ds_bpermute), flipping the k-mer on a reverse read (flip_k_strand)
 *      and searching the base_to_event_map for the closest event (get_closest_event_to, meth.c:100-125);
 *   2. the CpG sites of the disambiguated segment (meth.c:292-310: an IUPAC code becomes the first of its bases), 64 bytes per
 *      step, compacted by ballot + popcount;
 *   3. the groups (a new one where the gap is > 10, meth.c:496-512): a site starts a group by ballot, an end lane finds its
 *      group's first site as the highest start bit at or below it (or the carry from earlier steps) and evaluates its group:
 *      the skips of :521-523, the lower-bound search of find_by_ref_bounds (:425-470) in the record and the skips of :546-553;
 *   4. emit (second launch): the surviving groups' records and sequences, the wave writing one group's two sequences at a time.
 * The host launches the kernel twice (count, then emit into the slots the counts give).  Every index into the read's arrays is
 * bounded by the read's own sizes; CIGAR ops other than M I D S H = X mark the read and stop it. */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "abea_meth.h"

/* toupper, then getPossibleSymbols(c)[0] (meth.c:226-262); 0 = not an IUPAC code */
static __device__ __forceinline__ char meth_disambiguate(unsigned char c) {
    if (c >= 'a' && c <= 'z') c = (unsigned char)(c - 32);
    switch (c) {
        case 'A': case 'M': case 'R': case 'W': case 'V': case 'H': case 'D': case 'N': return 'A';
        case 'C': case 'S': case 'Y': case 'B': return 'C';
        case 'G': case 'K': return 'G';
        case 'T': return 'T';
        default: return 0;
    }
}
static __device__ __forceinline__ char meth_complement(char c) {   /* complement_dna[rank_dna[c]] on A, C, G, T */
    return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A';
}
/* inclusive prefix sum over the 64 lanes */
static __device__ __forceinline__ int wave_scan(int v, int lane) {
    for (int d = 1; d < 64; d <<= 1) {
        const int u = __shfl_up(v, d, 64);
        if (lane >= d) v += u;
    }
    return v;
}
/* get_next_event (meth.c:100-111): walks from start towards stop and never visits stop itself */
static __device__ __forceinline__ int meth_next_event(const int32_t* __restrict__ map, int start, int stop, int stride) {
    while (stride > 0 ? start < stop : start > stop) {
        const int ei = map[start];
        if (ei != -1) return ei;
        start += stride;
    }
    return -1;
}
/* aligned_pair_lower_bound (meth.c:414-423) over the record's reference positions (rec[2 i]) */
static __device__ __forceinline__ int meth_lower_bound(const int32_t* rec, int n, int v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (rec[2 * mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

extern "C" __global__ __launch_bounds__(256)
void abea_meth_sites_kernel(int n_reads, int emit, int k, const abea_meth_read* __restrict__ reads, const char* __restrict__ segs,
                            const uint32_t* __restrict__ cigars, const int32_t* __restrict__ maps, int32_t* scratch,
                            abea_meth_count* __restrict__ counts, abea_meth_group* __restrict__ groups, char* __restrict__ seqs) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_reads) return;
    const int lane = threadIdx.x & 63;
    const unsigned long long lt = (1ull << lane) - 1ull;
    const abea_meth_read R = reads[r];
    const char* __restrict__ seg = segs + R.seg_off;
    const uint32_t* __restrict__ cig = cigars + R.cigar_off;
    const int32_t* __restrict__ map = maps + R.map_off;
    int32_t* sites = scratch + R.scratch_off;
    int32_t* rec = sites + (R.seg_len / 2 + 1);                 /* {ref_pos, event_idx} pairs, at most read_len of them */
    const int S = R.seg_len, L = R.read_len, rc = R.rc;
    int err = 0;

    /* ---- 1. the event-alignment record (get_event_alignment_record, meth.c:127-185) ---- */
    int read_carry = 0, ref_carry = R.pos, n_rec = 0;
    const int map_size = L - k + 1;
    for (int base = 0; base < R.n_cigar; base += 64) {
        const int i = base + lane;
        int op = 5, len = 0;                                        /* lanes past the end: H of length 0 */
        if (i < R.n_cigar) { const uint32_t w = cig[i]; op = (int)(w & 15u); len = (int)(w >> 4); }
        if (__ballot(op == 3 || op == 6 || op > 8)) { err |= ABEA_METH_ERR_CIGAR; break; }   /* N, P or unknown: meth.c:60-73 */
        const bool aligned = op == 0 || op == 7 || op == 8;
        const int rinc = (aligned || op == 1 || op == 4) ? len : 0;
        const int finc = (aligned || op == 2) ? len : 0;
        const int rs = wave_scan(rinc, lane), fs = wave_scan(finc, lane);
        const int read0 = read_carry + rs - rinc, ref0 = ref_carry + fs - finc;
        /* the kept positions of the op: k <= read_pos and read_pos + k < read_len (meth.c:150-156) */
        const int lo = max(read0, k), hi = min(read0 + len, L - k);
        const int cnt = (aligned && hi > lo) ? hi - lo : 0;
        const int cs = wave_scan(cnt, lane);
        const int cs_ex = cs - cnt, ref_lo = ref0 + (lo - read0);
        const int total = __shfl(cs, 63, 64);
        for (int p0 = 0; p0 < total; p0 += 64) {
            const int p = p0 + lane;
            int a = 0, b = 63;                                      /* the first op j with cs_j > p */
            for (int s = 0; s < 6; ++s) {
                const int mid = (a + b) >> 1;
                const int v = __shfl(cs, mid, 64);
                if (a < b) { if (v > p) b = mid; else a = mid + 1; }
            }
            const int jlo = __shfl(lo, a, 64), jref = __shfl(ref_lo, a, 64), jex = __shfl(cs_ex, a, 64);
            const int slot = n_rec + p;
            if (p < total && slot < L) {
                const int t = p - jex, read_pos = jlo + t;
                const int kidx = rc ? L - read_pos - k : read_pos;   /* flip_k_strand (meth.c:122-125) */
                /* get_closest_event_to: index 0 is never searched backwards, map_size - 1 never forwards (stop is not visited) */
                const int before = meth_next_event(map, kidx, max(0, kidx - 1000), -1);
                const int after = meth_next_event(map, kidx, min(kidx + 1000, map_size - 1), 1);
                rec[2 * slot] = jref + t;
                rec[2 * slot + 1] = before == -1 ? after : before;
            }
        }
        read_carry += __shfl(rs, 63, 64);
        ref_carry += __shfl(fs, 63, 64);
        n_rec = min(n_rec + total, L);
    }

    /* ---- 2. CpG sites of the disambiguated segment (meth.c:481-491) ---- */
    int n_sites = 0;
    if (!err) {
        for (int base = 0; base < S; base += 64) {
            const int i = base + lane;
            const char c0 = i < S ? meth_disambiguate((unsigned char)seg[i]) : 'A';
            const char c1 = i + 1 < S ? meth_disambiguate((unsigned char)seg[i + 1]) : 'A';
            if (__ballot(c0 == 0)) { err |= ABEA_METH_ERR_BASE; break; }
            const bool is = i + 1 < S && c0 == 'C' && c1 == 'G';
            const unsigned long long m = __ballot(is);
            if (is) sites[n_sites + __popcll(m & lt)] = i;
            n_sites += __popcll(m);
        }
    }
    /* the record and the sites were written by other lanes of this wave: make them visible to its loads */
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_s_waitcnt(0);
    if (err) {
        if (lane == 0) { counts[r].n_groups = 0; counts[r].n_skipped = 0; counts[r].error = err; }
        return;
    }
    if (n_rec > 0 && rec[1] == rec[2 * n_rec - 1]) n_rec = 0;      /* degenerate alignment (meth.c:176-183) */

    /* ---- 3. groups, their bounds and skips; 4. emit ---- */
    int carry_start = 0, n_out = 0, n_skip = 0;
    for (int base = 0; base < n_sites; base += 64) {
        const int j = base + lane;
        const bool valid = j < n_sites;
        const int s = valid ? sites[j] : 0;
        const bool is_start = valid && (j == 0 || s - sites[j - 1] > ABEA_METH_SEP);
        const bool is_end = valid && (j == n_sites - 1 || sites[j + 1] - s > ABEA_METH_SEP);
        const unsigned long long sm = __ballot(is_start);
        const unsigned long long le = sm & (lt | (1ull << lane));
        const int my_start = le ? base + 63 - __clzll(le) : carry_start;
        if (sm) carry_start = base + 63 - __clzll(sm);
        bool survive = false, skipped = false;
        int e1 = 0, e2 = 0, first = 0, sub_start = 0, seq_len = 0;
        if (is_end) {
            first = sites[my_start];
            sub_start = first - ABEA_METH_SEP;
            const int sub_end = s + ABEA_METH_SEP, span = s - first;
            if (!(sub_start <= ABEA_METH_SEP || span > ABEA_METH_MAX_SPAN)) {         /* meth.c:521-523 */
                const int cs = sub_start + R.pos, ce = sub_end + R.pos;
                const int si = meth_lower_bound(rec, n_rec, cs), ti = meth_lower_bound(rec, n_rec, ce);
                /* left_bounded (meth.c:441-443): after a lower bound, true unless si == 0 and rec[0] lies past the start;
                 * right_bounded is always true after a lower bound (the reference's pairs[stop + 1] is not read) */
                if (si < n_rec && ti < n_rec && (si != 0 || rec[0] <= cs)) {
                    e1 = rec[2 * si + 1]; e2 = rec[2 * ti + 1];
                    /* the ratio test of meth.c:547 divides by calling_start - calling_end < 0: it never rejects */
                    if (abs(e2 - e1) > 10) {
                        const bool rev = e1 > e2;
                        /* the reference passes a bound of -1 as (uint32_t)-1 into the HMM, or asserts on a stride against
                         * the strand (hmm.c:331): skipped and counted here */
                        if (e1 < 0 || e2 < 0 || e1 >= R.n_events || e2 >= R.n_events || rev != (rc != 0)) skipped = true;
                        else survive = true;
                        seq_len = min(sub_end - sub_start + 1, S - sub_start);   /* std::string::substr clamps */
                    }
                }
            }
        }
        const unsigned long long vm = __ballot(survive);
        n_skip += __popcll(__ballot(skipped));
        if (emit) {
            const int idx = n_out + __popcll(vm & lt);
            if (survive) {
                abea_meth_group g;
                g.e1 = e1; g.e2 = e2; g.start = first + R.pos; g.end = s + R.pos; g.n_cpg = j - my_start + 1;
                g.seq_len = seq_len; g.pad0 = 0; g.pad1 = 0;
                groups[R.group_off + idx] = g;
            }
            for (unsigned long long mm = vm; mm; mm &= mm - 1) {   /* one group at a time, the wave over its bases */
                const int src = __ffsll((long long)mm) - 1;
                const int g_sub = __shfl(sub_start, src, 64), g_len = __shfl(seq_len, src, 64), g_idx = __shfl(idx, src, 64);
                char* u = seqs + (R.group_off + g_idx) * (int64_t)(2 * ABEA_METH_SEQ_SLOT);
                char* m = u + ABEA_METH_SEQ_SLOT;
                const char* sub = seg + g_sub;
                for (int t = lane; t <= g_len; t += 64) {
                    if (t == g_len) { u[t] = 0; m[t] = 0; continue; }
                    if (!rc) {                                      /* subseq, methylate(subseq) (meth.c:354-377) */
                        const char c = meth_disambiguate((unsigned char)sub[t]);
                        const bool cpg = c == 'C' && t + 1 < g_len && meth_disambiguate((unsigned char)sub[t + 1]) == 'G';
                        u[t] = c; m[t] = cpg ? 'M' : c;
                    } else {                                        /* reverse_complement, reverse_complement_meth(methylate) */
                        const int x = g_len - 1 - t;
                        const char c = meth_disambiguate((unsigned char)sub[x]);
                        const bool cpg = c == 'G' && x >= 1 && meth_disambiguate((unsigned char)sub[x - 1]) == 'C';
                        u[t] = meth_complement(c); m[t] = cpg ? 'M' : meth_complement(c);
                    }
                }
            }
        }
        n_out += __popcll(vm);
    }
    if (lane == 0) { counts[r].n_groups = n_out; counts[r].n_skipped = n_skip; counts[r].error = 0; }
}
