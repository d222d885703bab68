/* tests/fields_driver.cpp — a plain g++ caller shaped like f5c's resquiggle (process_db_rsq + output_db_rsq,
 * src/resquiggle.c:283-449) that asks for the event-table fields resquiggle reads and no more: the same batch (the dump format of
 * tests/process_driver.cpp, mode 0) through
 *   abea_f5c_process_fields(..., ABEA_EV_FIELDS_LAYOUT)   start + length of every event
 *   abea_f5c_process(...)                                 every field (ABEA_EV_FIELDS_ALL)
 * each from the raw float ADC counts (the shim leaves them in pA, so every call starts from a fresh copy), and writes for both:
 *   <out>.<sel>.events  binary: per read u64 n, then n event_t
 *   <out>.<sel>.tsv / .paf  abea_rsq_format_batch, fmt 0 / 1
 *   <out>.<sel>.state   text: i flag n_event_alignment events_per_base shift scale var log_var n_pairs (floats as %a), map
 *   <out>.bytes         text: d2h bytes of the LAYOUT call, of the ALL call, total events */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../include/abea_f5c_shim.h"

static std::vector<char> slurp(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
    std::vector<char> b((size_t)n);
    if (fread(b.data(), 1, (size_t)n, f) != (size_t)n) { perror("fread"); exit(2); }
    fclose(f);
    return b;
}
static FILE* open_out(const std::string& base, const char* ext, const char* mode) {
    FILE* f = fopen((base + ext).c_str(), mode);
    if (!f) { perror(ext); exit(2); }
    return f;
}

struct outputs {
    std::vector<abea_f5c_event_table> et;
    std::vector<abea_scalings_t> sc;
    std::vector<abea_pair_t*> pairs;
    std::vector<int32_t> n_pairs, flag, nal;
    std::vector<abea_index_pair_t*> b2e;
    std::vector<double> epb;
    uint64_t d2h = 0;
};

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s batch.bin out_prefix\n", argv[0]); return 2; }
    std::vector<char> buf = slurp(argv[1]);
    const std::string out = argv[2];
    const char* p = buf.data();
    int32_t hdr[6]; memcpy(hdr, p, 24); p += 24;            /* n_reads, kmer_size, n_model, mode, rna, pad */
    const int32_t n = hdr[0]; const uint32_t k = (uint32_t)hdr[1]; const int32_t n_model = hdr[2], mode = hdr[3], rna = hdr[4];
    if (mode != 0) { fprintf(stderr, "raw-signal batches only (mode 0)\n"); return 2; }
    const abea_model_t* model = (const abea_model_t*)p; p += (size_t)n_model * sizeof(abea_model_t);
    std::vector<int32_t> read_len(n); memcpy(read_len.data(), p, 4 * (size_t)n); p += 4 * (size_t)n;
    std::vector<int64_t> nsample(n); memcpy(nsample.data(), p, 8 * (size_t)n); p += 8 * (size_t)n;
    std::vector<float> offset(n), range(n), digit(n);
    for (int32_t i = 0; i < n; ++i) { float t[3]; memcpy(t, p, 12); p += 12; offset[i] = t[0]; range[i] = t[1]; digit[i] = t[2]; }
    std::vector<std::string> ids(n);
    for (int32_t i = 0; i < n; ++i) { ids[i] = std::string(p, strnlen(p, 40)); p += 40; }
    std::vector<char*> read(n);
    for (int32_t i = 0; i < n; ++i) {
        read[i] = (char*)malloc((size_t)read_len[i] + 1);
        memcpy(read[i], p, (size_t)read_len[i]); read[i][read_len[i]] = 0; p += read_len[i];
    }
    std::vector<std::vector<float>> adc(n);                  /* the ADC counts as f5c holds them (f5c.h:276-286) */
    for (int32_t i = 0; i < n; ++i) {
        if (nsample[i] <= 0) continue;
        adc[i].resize((size_t)nsample[i]);
        memcpy(adc[i].data(), p, 4 * (size_t)nsample[i]); p += 4 * (size_t)nsample[i];
    }

    abea_f5c_core core; memset(&core, 0, sizeof core);
    core.model = model; core.kmer_size = k; core.cuda_dev_id = 0; core.cuda_mem_frac = 0.2f; core.verbosity = 1; core.rna = rna;
    abea_f5c_init(&core);
    outputs o[2];                                            /* 0: LAYOUT, 1: ALL */
    const char* sel[2] = {"layout", "all"};
    std::vector<const char*> idp(n);
    for (int32_t i = 0; i < n; ++i) idp[i] = ids[i].c_str();
    for (int s = 0; s < 2; ++s) {
        outputs& r = o[s];
        std::vector<float*> raw(n, nullptr);
        for (int32_t i = 0; i < n; ++i) if (nsample[i] > 0) { raw[i] = (float*)malloc(4 * (size_t)nsample[i]); memcpy(raw[i], adc[i].data(), 4 * (size_t)nsample[i]); }
        r.et.assign((size_t)n, abea_f5c_event_table()); r.sc.assign((size_t)n, abea_scalings_t());
        r.pairs.assign((size_t)n, nullptr); r.n_pairs.assign((size_t)n, -1); r.flag.assign((size_t)n, 0); r.nal.assign((size_t)n, 0);
        r.b2e.assign((size_t)n, nullptr); r.epb.assign((size_t)n, 0.0);
        abea_f5c_db db; memset(&db, 0, sizeof db);           /* the glue of INTEGRATION.md, on stand-in arrays */
        db.n_bam_rec = n; db.read = read.data(); db.read_len = read_len.data(); db.nsample = nsample.data(); db.et = r.et.data();
        db.scalings = r.sc.data(); db.event_align_pairs = r.pairs.data(); db.n_event_align_pairs = r.n_pairs.data();
        db.base_to_event_map = r.b2e.data(); db.events_per_base = r.epb.data(); db.read_stat_flag = r.flag.data();
        db.n_event_alignment = r.nal.data();
        db.rawptr = raw.data(); db.offset = offset.data(); db.range = range.data(); db.digitisation = digit.data();
        for (int32_t i = 0; i < n; ++i) db.sum_bases += read_len[i];
        if (s == 0) abea_f5c_process_fields(&core, &db, ABEA_EV_FIELDS_LAYOUT);
        else abea_f5c_process(&core, &db);
        abea_stats st;
        abea_get_stats((abea_ctx*)core.cuda, &st);
        r.d2h = (uint64_t)st.d2h_bytes;
        for (int32_t i = 0; i < n; ++i) free(raw[i]);

        const std::string base = out + "." + sel[s];
        FILE* f = open_out(base, ".events", "wb");
        for (int32_t i = 0; i < n; ++i) {
            const uint64_t ne = r.et[i].n;
            fwrite(&ne, 8, 1, f);
            if (ne) fwrite(r.et[i].event, sizeof(abea_event_t), (size_t)ne, f);
        }
        fclose(f);
        f = open_out(base, ".state", "w");
        for (int32_t i = 0; i < n; ++i) {
            fprintf(f, "%d\t%d\t%d\t%a\t%a\t%a\t%a\t%a\t%d\t", i, r.flag[i], r.nal[i], r.epb[i], (double)r.sc[i].shift, (double)r.sc[i].scale,
                    (double)r.sc[i].var, (double)r.sc[i].log_var, r.n_pairs[i]);
            for (int32_t j = 0; j < r.n_pairs[i] && r.pairs[i]; ++j) fprintf(f, "{%d,%d}", r.pairs[i][j].ref_pos, r.pairs[i][j].read_pos);
            fprintf(f, "\t");
            if (r.b2e[i]) for (int32_t j = 0; j < read_len[i] - (int32_t)k + 1; ++j) fprintf(f, "%d,%d ", r.b2e[i][j].start, r.b2e[i][j].stop);
            else fprintf(f, "NULL");
            fprintf(f, "\n");
        }
        fclose(f);
        std::vector<const abea_event_t*> evp(n);
        for (int32_t i = 0; i < n; ++i) evp[i] = r.et[i].event;
        for (int fmt = 0; fmt < 2; ++fmt) {                  /* output_db_rsq, both formats (size query first, then the text) */
            int32_t printed = 0;
            const int64_t len = abea_rsq_format_batch(nullptr, 0, fmt, n, idp.data(), read_len.data(), k, r.b2e.data(), evp.data(),
                                                      nsample.data(), r.sc.data(), r.flag.data(), rna, &printed);
            if (len < 0) { fprintf(stderr, "abea_rsq_format_batch failed: %lld\n", (long long)len); return 3; }
            std::vector<char> text((size_t)len + 1);
            abea_rsq_format_batch(text.data(), text.size(), fmt, n, idp.data(), read_len.data(), k, r.b2e.data(), evp.data(),
                                  nsample.data(), r.sc.data(), r.flag.data(), rna, &printed);
            f = open_out(base, fmt ? ".paf" : ".tsv", "w");
            fwrite(text.data(), 1, (size_t)len, f);
            fclose(f);
        }
    }
    uint64_t n_ev = 0;
    for (int32_t i = 0; i < n; ++i) n_ev += o[1].et[i].n;
    FILE* f = open_out(out, ".bytes", "w");
    fprintf(f, "%llu %llu %llu\n", (unsigned long long)o[0].d2h, (unsigned long long)o[1].d2h, (unsigned long long)n_ev);
    fclose(f);
    fprintf(stderr, "d2h bytes: LAYOUT %llu, ALL %llu, %llu events\n", (unsigned long long)o[0].d2h, (unsigned long long)o[1].d2h,
            (unsigned long long)n_ev);
    abea_f5c_free(&core);
    for (int s = 0; s < 2; ++s)
        for (int32_t i = 0; i < n; ++i) { free(o[s].et[i].event); free(o[s].pairs[i]); free(o[s].b2e[i]); }
    for (int32_t i = 0; i < n; ++i) free(read[i]);
    return 0;
}
