/* abea_meth.cpp — host driver of call-methylation, mode 0 (meth_single -> calculate_methylation_for_read, reference
 * src/meth.c:473-612, called from src/f5c.c:885-890) and the text of output_db for it (f5c.c:1033-1062).
 *
 * Per chunk of reads: flatten (worker pool) the segments, CIGARs, map starts and event means into pinned staging and copy them
 * up once; abea_meth_sites_kernel counts the surviving CpG groups of every read; one small copy down of the counts gives every
 * read its slots; the same kernel emits the group records and sequences into them; the records come down, and the host orders
 * the jobs (at most 16 k-mers first, as abea_hmm_forward_kernel's grid needs) and writes their descriptors with the read's
 * transition log-probabilities (glibc logf, as abea_hmm.cpp); abea_hmm_forward_kernel scores them.  A job's event window is
 * read in place from its read's means, which go up in the order the job walks them (reversed on a reverse read, whose jobs
 * run with stride -1), so no window is copied.  No CPU fallback. */
#include <string>
#include <thread>
#include "abea_internal.h"
#include "abea_hmm.h"
#include "abea_meth.h"

extern "C" __global__ void abea_meth_sites_kernel(int, int, int, const abea_meth_read*, const char*, const uint32_t*, const int32_t*,
                                                  int32_t*, abea_meth_count*, abea_meth_group*, char*);
extern "C" __global__ void abea_hmm_forward_kernel(int, int, int, const abea_hmm_job*, const char*, const float*,
                                                   const abea_model_t*, int, const float*, const float*, float*, float*);

namespace {

struct meth_read_info { int32_t seg_len; bool active; };

static const int ABEA_METH_RETRY = 1;          /* chunk_run: the chunk's jobs do not fit the arena, split it */

/* bytes of the inputs and scratch of one read in the arena (what the count pass needs) */
size_t read_bytes(const abea_meth_batch* B, int32_t i, const meth_read_info& m, uint32_t k) {
    const int64_t L = std::max(B->read_len[i], 0), K = std::max<int64_t>(L - (int64_t)k + 1, 0);
    return sizeof(abea_meth_read) + align_up((size_t)m.seg_len + 1, 4) + 4 * (size_t)B->n_cigar[i] + 4 * (size_t)K +
           4 * (size_t)B->n_events[i] + 4 * ((size_t)m.seg_len / 2 + 1 + 2 * (size_t)L) + sizeof(abea_meth_count);
}

struct meth_call {
    const abea_meth_batch* B;
    const abea_model_t* cpgmodel;
    uint32_t k;
    std::vector<meth_read_info>* info;
};

int chunk_run(abea_ctx* c, const meth_call& M, const int32_t* ids, int32_t n, abea_stats& st) {
    const abea_meth_batch* B = M.B;
    const uint32_t k = M.k;
    abea_hmm_state* S = c->hmm;
    const std::vector<meth_read_info>& info = *M.info;
    const double t0 = abea_now_ms();
    /* ---- layout of the inputs ---- */
    std::vector<abea_meth_read> rd((size_t)n);
    std::vector<int64_t> mean_off((size_t)n);                   /* floats: the read's event means (reversed on a reverse read) */
    size_t seg_b = 0, cig_w = 0, map_w = 0, ev_w = 0, scr_w = 0;
    for (int32_t q = 0; q < n; ++q) {
        const int32_t i = ids[q];
        abea_meth_read& d = rd[(size_t)q];
        memset(&d, 0, sizeof d);
        const int32_t L = std::max(B->read_len[i], 0);
        d.seg_len = info[(size_t)i].seg_len; d.read_len = L; d.n_cigar = (int32_t)B->n_cigar[i];
        d.n_events = (int32_t)B->n_events[i]; d.pos = B->pos[i]; d.rc = B->is_rev[i] ? 1 : 0;
        d.seg_off = (int64_t)seg_b;     seg_b += align_up((size_t)d.seg_len + 1, 4);
        d.cigar_off = (int64_t)cig_w;   cig_w += (size_t)d.n_cigar;
        d.map_off = (int64_t)map_w;     map_w += (size_t)std::max<int64_t>((int64_t)L - k + 1, 0);
        mean_off[(size_t)q] = (int64_t)ev_w; ev_w += (size_t)d.n_events;
        d.scratch_off = (int64_t)scr_w; scr_w += (size_t)d.seg_len / 2 + 1 + 2 * (size_t)L;
        d.group_off = 0;                                        /* set from the counts, before the emit pass */
    }
    size_t o = 0;
    const size_t o_rd = o;   o = align_up(o + (size_t)n * sizeof(abea_meth_read), 256);
    const size_t o_seg = o;  o = align_up(o + seg_b, 256);
    const size_t o_cig = o;  o = align_up(o + cig_w * 4, 256);
    const size_t o_map = o;  o = align_up(o + map_w * 4, 256);
    const size_t o_ev = o;   o = align_up(o + ev_w * 4, 256);
    const size_t up_bytes = o;
    const size_t o_cnt = o;  o = align_up(o + (size_t)n * sizeof(abea_meth_count), 256);
    const size_t o_scr = o;  o = align_up(o + scr_w * 4, 256);
    const size_t o_tail = o;
    if (o_tail + 4096 > c->arena_bytes) return n > 1 ? ABEA_METH_RETRY : abea_fail(ABEA_ENOMEM, "read %d does not fit the arena", ids[0]);
    int rc = ensure_pinned((void**)&S->mpin, &S->mpin_cap, std::max(up_bytes, (size_t)n * sizeof(abea_meth_count)));
    if (rc) return rc;
    uint8_t* pin = S->mpin;
    abea_parallel_for(c, n, 64, [&](int64_t lo, int64_t hi) {
        for (int64_t q = lo; q < hi; ++q) {
            const int32_t i = ids[q];
            const abea_meth_read& d = rd[(size_t)q];
            memcpy(pin + o_seg + d.seg_off, B->fasta_cache[i], (size_t)d.seg_len + 1);
            if (d.n_cigar) memcpy(pin + o_cig + 4 * d.cigar_off, B->cigar[i], 4 * (size_t)d.n_cigar);
            int32_t* mp = (int32_t*)(pin + o_map) + d.map_off;
            const int64_t K = std::max<int64_t>((int64_t)d.read_len - k + 1, 0);
            for (int64_t j = 0; j < K; ++j) mp[j] = B->base_to_event_map[i][j].start;
            float* ev = (float*)(pin + o_ev) + mean_off[(size_t)q];
            const abea_event_t* e = B->events[i];
            const int32_t E = d.n_events;
            if (d.rc) for (int32_t j = 0; j < E; ++j) ev[j] = e[E - 1 - j].mean;   /* a reverse read's jobs walk it downwards */
            else for (int32_t j = 0; j < E; ++j) ev[j] = e[j].mean;
        }
    });
    memcpy(pin + o_rd, rd.data(), (size_t)n * sizeof(abea_meth_read));
    st.flatten_ms += abea_now_ms() - t0;
    uint8_t* dev = c->arena;
    HIP_TRY(hipMemcpyAsync(dev, pin, up_bytes, hipMemcpyHostToDevice, c->stream));
    st.h2d_bytes += up_bytes;
    const unsigned blocks = (unsigned)((n + 3) / 4);
    HIP_TRY(hipEventRecord(S->m0, c->stream));
    hipLaunchKernelGGL(abea_meth_sites_kernel, dim3(blocks), dim3(256), 0, c->stream, (int)n, 0, (int)k,
                       (const abea_meth_read*)(dev + o_rd), (const char*)(dev + o_seg), (const uint32_t*)(dev + o_cig),
                       (const int32_t*)(dev + o_map), (int32_t*)(dev + o_scr), (abea_meth_count*)(dev + o_cnt),
                       (abea_meth_group*)nullptr, (char*)nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(S->m1, c->stream));
    std::vector<abea_meth_count> cnt((size_t)n);
    HIP_TRY(hipMemcpyAsync(pin, dev + o_cnt, (size_t)n * sizeof(abea_meth_count), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    memcpy(cnt.data(), pin, (size_t)n * sizeof(abea_meth_count));
    st.d2h_bytes += (uint64_t)n * sizeof(abea_meth_count);
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, S->m0, S->m1));
    st.meth_ms += ms;
    int64_t G = 0, skipped = 0;
    for (int32_t q = 0; q < n; ++q) {
        if (cnt[(size_t)q].error)
            return abea_fail(ABEA_EINVAL, "read %d: %s", ids[q], (cnt[(size_t)q].error & ABEA_METH_ERR_CIGAR)
                             ? "the CIGAR holds N (ref skip) or an op get_aligned_segments does not handle"
                             : "the reference segment holds a byte that is no IUPAC code");
        rd[(size_t)q].group_off = G;
        G += cnt[(size_t)q].n_groups;
        skipped += cnt[(size_t)q].n_skipped;
    }
    if (G == 0) { st.meth_groups_skipped += skipped; st.n_sub_batches += 1; return ABEA_OK; }
    /* ---- emit ---- */
    o = o_tail;
    const size_t o_grp = o;  o = align_up(o + (size_t)G * sizeof(abea_meth_group), 256);
    const size_t o_seq = o;  o = align_up(o + (size_t)G * 2 * ABEA_METH_SEQ_SLOT, 256);
    if ((size_t)G * 2 * ABEA_METH_SEQ_SLOT > (size_t)INT32_MAX || o + 4096 > c->arena_bytes)   /* seq_off is 32-bit in the job */
        return n > 1 ? ABEA_METH_RETRY : abea_fail(ABEA_ENOMEM, "read %d: %lld CpG groups do not fit the arena", ids[0], (long long)G);
    rc = ensure_pinned((void**)&S->mpin, &S->mpin_cap, std::max((size_t)n * sizeof(abea_meth_read), (size_t)G * sizeof(abea_meth_group)));
    if (rc) return rc;                                            /* (the stream is idle here and below: no copy reads the old block) */
    pin = S->mpin;
    memcpy(pin, rd.data(), (size_t)n * sizeof(abea_meth_read));
    HIP_TRY(hipMemcpyAsync(dev + o_rd, pin, (size_t)n * sizeof(abea_meth_read), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(S->m0, c->stream));
    hipLaunchKernelGGL(abea_meth_sites_kernel, dim3(blocks), dim3(256), 0, c->stream, (int)n, 1, (int)k,
                       (const abea_meth_read*)(dev + o_rd), (const char*)(dev + o_seg), (const uint32_t*)(dev + o_cig),
                       (const int32_t*)(dev + o_map), (int32_t*)(dev + o_scr), (abea_meth_count*)(dev + o_cnt),
                       (abea_meth_group*)(dev + o_grp), (char*)(dev + o_seq));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(S->m1, c->stream));
    std::vector<abea_meth_group> grp((size_t)G);
    HIP_TRY(hipMemcpyAsync(pin, dev + o_grp, (size_t)G * sizeof(abea_meth_group), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    memcpy(grp.data(), pin, (size_t)G * sizeof(abea_meth_group));
    st.d2h_bytes += (uint64_t)G * sizeof(abea_meth_group);
    HIP_TRY(hipEventElapsedTime(&ms, S->m0, S->m1));
    st.meth_ms += ms;
    /* ---- jobs: 2 per group (unmethylated 2g, methylated 2g + 1), at most 16 k-mers first ---- */
    const double t1 = abea_now_ms();
    const int64_t NJ = 2 * G;
    /* launch order (serial, integer only): a group's two jobs go to the narrow part when they have at most 16 k-mers; the column
     * scratch of jobs with more than 64 k-mers */
    std::vector<int64_t> slot((size_t)G), col((size_t)G);
    int64_t n16 = 0;
    int32_t max_ev = 0;
    for (int64_t g = 0; g < G; ++g) {
        const abea_meth_group& x = grp[(size_t)g];
        n16 += 2 * (((int64_t)x.seq_len - k + 1) <= 16);
        max_ev = std::max(max_ev, std::abs(x.e2 - x.e1) + 1);
    }
    size_t tot_col = 0;
    for (int64_t g = 0, a = 0, b = n16; g < G; ++g) {
        const abea_meth_group& x = grp[(size_t)g];
        const int64_t nk = (int64_t)x.seq_len - k + 1;
        if (nk <= 16) { slot[(size_t)g] = a; a += 2; } else { slot[(size_t)g] = b; b += 2; }
        col[(size_t)g] = (int64_t)tot_col;
        if (nk > 64) tot_col += 2 * 3 * ((size_t)std::abs(x.e2 - x.e1) + 2);
    }
    std::vector<float> flank;
    abea_hmm_flank(flank, max_ev);
    const size_t o_desc = o; o = align_up(o + (size_t)NJ * sizeof(abea_hmm_job), 256);
    const size_t o_flank = o; o = align_up(o + flank.size() * 4, 256);
    const size_t o_out = o;  o = align_up(o + (size_t)NJ * 4, 256);
    const size_t o_col = o;  o = align_up(o + tot_col * 4, 256);
    if (o + 4096 > c->arena_bytes)
        return n > 1 ? ABEA_METH_RETRY : abea_fail(ABEA_ENOMEM, "read %d: its HMM jobs do not fit the arena", ids[0]);
    const size_t jb = o_out - o_desc;
    rc = ensure_pinned((void**)&S->mpin, &S->mpin_cap, std::max(jb, (size_t)NJ * 4));
    if (rc) return rc;
    pin = S->mpin;
    abea_hmm_job* desc = (abea_hmm_job*)pin;
    /* the descriptors, written straight into the staging by the worker pool, a read at a time */
    abea_parallel_for(c, n, 16, [&](int64_t lo, int64_t hi) {
        for (int64_t q = lo; q < hi; ++q) {
            const int32_t i = ids[q];
            abea_hmm_job p;
            memset(&p, 0, sizeof p);
            p.scale = B->scalings[i].scale; p.shift = B->scalings[i].shift; p.var = B->scalings[i].var; p.log_var = B->scalings[i].log_var;
            p.flags = 3u;                                              /* HAF_ALLOW_PRE_CLIP | HAF_ALLOW_POST_CLIP, meth.c:559 */
            p.rc = rd[(size_t)q].rc;
            abea_hmm_transitions(B->events_per_base[i], p);
            for (int64_t g = rd[(size_t)q].group_off; g < rd[(size_t)q].group_off + cnt[(size_t)q].n_groups; ++g) {
                const abea_meth_group& x = grp[(size_t)g];
                for (int h = 0; h < 2; ++h) {                           /* h = 0: unmethylated, 1: methylated */
                    abea_hmm_job d = p;
                    d.seq_off = (int32_t)((2 * g + h) * ABEA_METH_SEQ_SLOT);
                    d.seq_len = x.seq_len;
                    d.n_events = std::abs(x.e2 - x.e1) + 1;             /* hmm.c:649-654 */
                    d.ev_off = mean_off[(size_t)q] + (d.rc ? (int64_t)rd[(size_t)q].n_events - 1 - x.e1 : (int64_t)x.e1);
                    d.out_idx = (int32_t)(2 * g + 1 - h);                /* scores[2g] = methylated, [2g + 1] = unmethylated */
                    d.col_off = col[(size_t)g] + h * 3 * ((int64_t)d.n_events + 1);
                    desc[slot[(size_t)g] + h] = d;
                }
            }
        }
    });
    memcpy(pin + (o_flank - o_desc), flank.data(), flank.size() * 4);
    st.plan_ms += abea_now_ms() - t1;
    HIP_TRY(hipMemcpyAsync(dev + o_desc, pin, jb, hipMemcpyHostToDevice, c->stream));
    st.h2d_bytes += jb;
    const int blocks16 = (int)((n16 + 15) / 16), blocks64 = (int)((NJ - n16 + 3) / 4);
    HIP_TRY(hipEventRecord(S->m1, c->stream));
    hipLaunchKernelGGL(abea_hmm_forward_kernel, dim3((unsigned)(blocks16 + blocks64)), dim3(256), 0, c->stream,
                       (int)n16, (int)NJ, blocks16, (const abea_hmm_job*)(dev + o_desc), (const char*)(dev + o_seq),
                       (const float*)(dev + o_ev), S->d_model, (int)k, S->d_tbl, (const float*)(dev + o_flank),
                       (float*)(dev + o_col), (float*)(dev + o_out));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(S->m2, c->stream));
    HIP_TRY(hipMemcpyAsync(pin, dev + o_out, (size_t)NJ * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    st.d2h_bytes += (uint64_t)NJ * 4;
    HIP_TRY(hipEventElapsedTime(&ms, S->m1, S->m2));
    st.meth_ms += ms; st.hmm_ms += ms;
    /* ---- sites ---- */
    const double t2 = abea_now_ms();
    const float* sc = (const float*)pin;
    for (int32_t q = 0; q < n; ++q) {
        const int32_t i = ids[q], ng = cnt[(size_t)q].n_groups;
        if (!ng) continue;
        abea_meth_site_t* s = (abea_meth_site_t*)malloc((size_t)ng * sizeof(abea_meth_site_t));
        if (!s) return abea_fail(ABEA_ENOMEM, "malloc of %d sites", ng);
        for (int32_t g = 0; g < ng; ++g) {
            const int64_t x = rd[(size_t)q].group_off + g;
            const abea_meth_group& r = grp[(size_t)x];
            s[g].start_position = r.start; s[g].end_position = r.end; s[g].n_cpg = r.n_cpg; s[g].strands_scored = 1;
            s[g].ll_methylated = sc[2 * x]; s[g].ll_unmethylated = sc[2 * x + 1];
        }
        B->sites[i] = s; B->n_sites[i] = ng;
    }
    st.unflatten_ms += abea_now_ms() - t2;
    st.meth_groups += G; st.meth_groups_skipped += skipped;
    st.n_sub_batches += 1;
    return ABEA_OK;
}

/* the reads ids[0..n) on ONE device context, in chunks of at most `cap` reads (ABEA_METH_CHUNK_READS) whose inputs fill at most a
 * quarter of the arena; a chunk whose jobs then do not fit is split in two */
int meth_run(abea_ctx* c, const meth_call& M, const int32_t* ids, int32_t n, abea_stats& st) {
    const double t0 = abea_now_ms();
    memset(&st, 0, sizeof st);
    HIP_TRY(hipSetDevice(c->device));
    int rc = abea_hmm_prepare(c, M.cpgmodel, M.k);
    if (rc) return rc;
    abea_hmm_state* S = c->hmm;
    for (hipEvent_t* e : {&S->m0, &S->m1, &S->m2}) if (!*e) HIP_TRY(hipEventCreate(e));
    int32_t cap = 16384;
    if (const char* e = getenv("ABEA_METH_CHUNK_READS")) cap = std::max(1, atoi(e));
    const size_t budget = c->arena_bytes / 4;
    std::vector<std::pair<int32_t, int32_t>> todo;                 /* [lo, hi) of ids, last = next */
    for (int32_t lo = 0; lo < n;) {
        int32_t hi = lo;
        size_t bytes = 0;
        while (hi < n && hi - lo < cap) {
            const size_t b = read_bytes(M.B, ids[hi], (*M.info)[(size_t)ids[hi]], M.k);
            if (hi > lo && bytes + b > budget) break;
            bytes += b; ++hi;
        }
        todo.push_back({lo, hi});
        lo = hi;
    }
    std::reverse(todo.begin(), todo.end());
    while (!todo.empty()) {
        const auto ch = todo.back(); todo.pop_back();
        rc = chunk_run(c, M, ids + ch.first, ch.second - ch.first, st);
        if (rc == ABEA_METH_RETRY) {
            const int32_t mid = ch.first + (ch.second - ch.first) / 2;
            todo.push_back({mid, ch.second}); todo.push_back({ch.first, mid});
            continue;
        }
        if (rc) return rc;
    }
    st.n_reads_gpu = n;
    st.arena_bytes = c->arena_bytes;
    st.total_ms = abea_now_ms() - t0;
    return ABEA_OK;
}

}  // namespace

extern "C" int abea_meth_batch_host(abea_ctx* c, const abea_meth_batch* B, const abea_model_t* cpgmodel, uint32_t kmer_size) {
    if (!c || !B || !cpgmodel || B->n_reads < 0) return abea_fail(ABEA_EINVAL, "abea_meth_batch_host: null argument");
    if (kmer_size < 1 || kmer_size > ABEA_MAX_KMER_SIZE) return abea_fail(ABEA_EINVAL, "kmer_size %u", kmer_size);
    const int32_t n = B->n_reads;
    if (n == 0) return ABEA_OK;
    if (!B->n_sites || !B->sites) return abea_fail(ABEA_EINVAL, "abea_meth_batch_host: null output array");
    for (int32_t i = 0; i < n; ++i) { B->sites[i] = nullptr; B->n_sites[i] = 0; }   /* before any exit: the error path frees these */
    if (!B->fasta_cache || !B->pos || !B->cigar || !B->n_cigar || !B->is_rev || !B->read_len || !B->events || !B->n_events ||
        !B->base_to_event_map || !B->scalings || !B->events_per_base)
        return abea_fail(ABEA_EINVAL, "abea_meth_batch_host: null input array");
    ABEA_API_ENTER(c, "abea_meth_batch_host");
    const double t0 = abea_now_ms();
    std::vector<meth_read_info> info((size_t)n);
    std::vector<int32_t> ids;
    int32_t bad = -1;
    for (int32_t i = 0; i < n; ++i) {
        meth_read_info& m = info[(size_t)i];
        m.active = !(B->read_stat_flag && B->read_stat_flag[i]);
        m.seg_len = 0;
        if (!m.active) continue;
        const int64_t K = (int64_t)B->read_len[i] - kmer_size + 1;
        if (!B->fasta_cache[i] || B->read_len[i] < 0 || B->n_events[i] > (uint64_t)INT32_MAX || (B->n_cigar[i] && !B->cigar[i]) ||
            (K > 0 && !B->base_to_event_map[i]) || (B->n_events[i] && !B->events[i])) { bad = i; break; }
        const size_t sl = strlen(B->fasta_cache[i]);
        if (sl > (size_t)INT32_MAX / 2) { bad = i; break; }
        m.seg_len = (int32_t)sl;
        ids.push_back(i);
    }
    if (bad >= 0) return abea_fail(ABEA_EINVAL, "abea_meth_batch_host: read %d has a null array or an out-of-range size", bad);
    meth_call M{B, cpgmodel, kmer_size, &info};
    abea_stats st; memset(&st, 0, sizeof st);
    int rc = ABEA_OK;
    if (c->children.empty()) {
        rc = meth_run(c, M, ids.data(), (int32_t)ids.size(), st);
    } else {
        /* a share per device, longest-processing-time first on the segment length, one host thread each */
        const int32_t nd = (int32_t)c->children.size(), na = (int32_t)ids.size();
        std::vector<int64_t> weight((size_t)na);
        for (int32_t q = 0; q < na; ++q) weight[(size_t)q] = info[(size_t)ids[(size_t)q]].seg_len + 1;
        std::vector<int32_t> bin_of((size_t)na);
        rc = abea_lpt_split(weight.data(), na, nd, bin_of.data());
        if (rc) return rc;
        std::vector<std::vector<int32_t>> share((size_t)nd);
        for (int32_t q = 0; q < na; ++q) share[(size_t)bin_of[(size_t)q]].push_back(ids[(size_t)q]);
        std::vector<abea_stats> sts((size_t)nd);
        std::vector<int> rcs((size_t)nd, 0);
        std::vector<std::string> errs((size_t)nd);
        std::vector<std::thread> th;
        for (int32_t d = 0; d < nd; ++d)
            th.emplace_back([&, d]() {
                rcs[(size_t)d] = meth_run(c->children[(size_t)d], M, share[(size_t)d].data(), (int32_t)share[(size_t)d].size(), sts[(size_t)d]);
                if (rcs[(size_t)d]) errs[(size_t)d] = abea_last_error();
            });
        for (auto& t : th) t.join();
        for (int32_t d = 0; d < nd && !rc; ++d)
            if (rcs[(size_t)d]) rc = abea_fail(rcs[(size_t)d], "device %d: %s", c->children[(size_t)d]->device, errs[(size_t)d].c_str());
        for (int32_t d = 0; d < nd; ++d) {
            const abea_stats& b = sts[(size_t)d];
            c->children[(size_t)d]->stats = b;
            st.meth_ms = std::max(st.meth_ms, b.meth_ms); st.hmm_ms = std::max(st.hmm_ms, b.hmm_ms);
            st.flatten_ms = std::max(st.flatten_ms, b.flatten_ms); st.plan_ms = std::max(st.plan_ms, b.plan_ms);
            st.unflatten_ms = std::max(st.unflatten_ms, b.unflatten_ms);
            st.n_reads_gpu += b.n_reads_gpu; st.n_sub_batches += b.n_sub_batches; st.meth_groups += b.meth_groups;
            st.meth_groups_skipped += b.meth_groups_skipped; st.h2d_bytes += b.h2d_bytes; st.d2h_bytes += b.d2h_bytes;
            st.arena_bytes += b.arena_bytes;
        }
        st.n_devices = nd;
    }
    if (rc) {
        for (int32_t i = 0; i < n; ++i) { free(B->sites[i]); B->sites[i] = nullptr; B->n_sites[i] = 0; }
        return rc;
    }
    if (!st.n_devices) st.n_devices = 1;
    st.n_reads_skipped = n - (int64_t)ids.size();
    st.host_threads = abea_pool_threads(c->children.empty() ? c : c->children[0]);
    st.total_ms = abea_now_ms() - t0;
    c->stats = st;
    return ABEA_OK;
}

/* ---- output_db, mode 0 (f5c.c:1033-1062) ---- */
namespace {
char disambiguate_host(char c) {                 /* toupper + getPossibleSymbols(c)[0] (meth.c:292-310) */
    switch (toupper((unsigned char)c)) {
        case 'A': case 'M': case 'R': case 'W': case 'V': case 'H': case 'D': case 'N': return 'A';
        case 'C': case 'S': case 'Y': case 'B': return 'C';
        case 'G': case 'K': return 'G';
        case 'T': return 'T';
        default: return 0;
    }
}
void appendf(std::string& s, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
void appendf(std::string& s, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    const int m = vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (m < (int)sizeof buf) { s.append(buf, (size_t)std::max(m, 0)); return; }
    std::string big((size_t)m + 1, '\0');
    va_start(ap, fmt);
    vsnprintf(&big[0], big.size(), fmt, ap);
    va_end(ap);
    s.append(big.data(), (size_t)m);
}
}  // namespace

extern "C" int64_t abea_meth_format_batch(char* out, size_t cap, int version, int header, int32_t n_reads,
                                          const char* const* contig, const char* const* read_name, const uint8_t* is_rev,
                                          const char* const* fasta_cache, const int32_t* pos, const int32_t* read_stat_flag,
                                          const int32_t* n_sites, const abea_meth_site_t* const* sites, uint32_t kmer_size,
                                          int32_t clip_start, int32_t clip_end, int64_t* n_printed) {
    if ((version != 1 && version != 2) || n_reads < 0 || (!out && cap) || kmer_size < 1 || kmer_size > ABEA_MAX_KMER_SIZE) return ABEA_EINVAL;
    if (n_reads && (!contig || !read_name || !is_rev || !fasta_cache || !pos || !n_sites || !sites)) return ABEA_EINVAL;
    std::string text;
    if (header)                                                   /* meth_main.c:560-570 */
        text += version == 1 ? "chromosome\tstart\tend\tread_name\tlog_lik_ratio\tlog_lik_methylated\tlog_lik_unmethylated\t"
                               "num_calling_strands\tnum_cpgs\tsequence\n"
                             : "chromosome\tstrand\tstart\tend\tread_name\tlog_lik_ratio\tlog_lik_methylated\tlog_lik_unmethylated\t"
                               "num_calling_strands\tnum_motifs\tsequence\n";
    int64_t printed = 0;
    const int64_t k = kmer_size;
    for (int32_t i = 0; i < n_reads; ++i) {
        if ((read_stat_flag && read_stat_flag[i]) || n_sites[i] <= 0) continue;
        if (!sites[i] || !fasta_cache[i] || !contig[i] || !read_name[i]) return ABEA_EINVAL;
        const int64_t seg_len = (int64_t)strlen(fasta_cache[i]);
        for (int32_t j = 0; j < n_sites[i]; ++j) {
            const abea_meth_site_t& ss = sites[i][j];
            const double m = ss.ll_methylated, u = ss.ll_unmethylated, diff = m - u;
            if ((clip_start != -1 && ss.start_position < clip_start) || (clip_end != -1 && ss.end_position >= clip_end)) continue;
            /* ss.sequence = ref_seq.substr(first - k + 1, last + k - (first - k + 1)), meth.c:589-593 (substr clamps at the end) */
            const int64_t a = (int64_t)ss.start_position - pos[i] - k + 1, b = std::min<int64_t>((int64_t)ss.end_position - pos[i] + k, seg_len);
            if (a < 0 || a > seg_len) return ABEA_EINVAL;
            std::string seq;
            for (int64_t x = a; x < b; ++x) seq += disambiguate_host(fasta_cache[i][x]);
            if (version == 1) appendf(text, "%s\t%d\t%d\t", contig[i], ss.start_position, ss.end_position);
            else appendf(text, "%s\t%c\t%d\t%d\t", contig[i], is_rev[i] ? '-' : '+', ss.start_position, ss.end_position);
            appendf(text, "%s\t%.2lf\t", read_name[i], diff);
            appendf(text, "%.2lf\t%.2lf\t", m, u);
            appendf(text, "%d\t%d\t%s\n", ss.strands_scored, ss.n_cpg, seq.c_str());
            ++printed;
        }
    }
    if (n_printed) *n_printed = printed;
    if (out && cap) {
        const size_t w = text.size() < cap - 1 ? text.size() : cap - 1;
        memcpy(out, text.data(), w);
        out[w] = '\0';
    }
    return (int64_t)text.size();
}
