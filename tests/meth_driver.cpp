// A plain g++ caller of call-methylation through the f5c shim (include/abea_f5c_shim.h: abea_f5c_init -> abea_f5c_meth -> abea_f5c_free)
// and of abea_meth_format_batch.  Input (written by tests/test_meth_gpu.py): int32 n, k, n_model; the nucleotide model (4^k entries)
// and the CpG model (5^k); per read int32 pos, is_rev, read_len, n_cigar, seg_len, n_events, read_stat_flag, 0, the CIGAR words, the
// segment, the event means (float32), the base_to_event_map starts (int32, read_len - k + 1 of them), the scalings (4 float32) and
// events_per_base (float64).  Output: <out>.sites = per read int32 n_sites and the abea_meth_site_t records; <out>.tsv = the text.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../include/abea_f5c_shim.h"

template <class T> static void rd(FILE* f, T* p, size_t n) {
    if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s input out_prefix\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[3];
    rd(f, hdr, 3);
    const int32_t n = hdr[0], k = hdr[1], n_model = hdr[2];
    size_t n_cpg = 1;
    for (int i = 0; i < k; ++i) n_cpg *= 5;
    std::vector<abea_model_t> model((size_t)n_model), cpg(n_cpg);
    rd(f, model.data(), model.size()); rd(f, cpg.data(), cpg.size());
    std::vector<int32_t> pos(n), read_len(n), flag(n);
    std::vector<uint32_t> n_cigar(n);
    std::vector<uint8_t> rev(n);
    std::vector<std::vector<uint32_t>> cig(n);
    std::vector<std::string> seg(n);
    std::vector<std::vector<abea_event_t>> ev(n);
    std::vector<std::vector<abea_index_pair_t>> map(n);
    std::vector<abea_scalings_t> sc(n);
    std::vector<double> epb(n);
    for (int32_t i = 0; i < n; ++i) {
        int32_t h[8];
        rd(f, h, 8);
        pos[i] = h[0]; rev[i] = (uint8_t)h[1]; read_len[i] = h[2]; n_cigar[i] = (uint32_t)h[3]; flag[i] = h[6];
        cig[i].resize((size_t)h[3]); rd(f, cig[i].data(), cig[i].size());
        seg[i].resize((size_t)h[4]); rd(f, &seg[i][0], seg[i].size());
        std::vector<float> m((size_t)h[5]); rd(f, m.data(), m.size());
        ev[i].assign(m.size(), abea_event_t{0, 0.f, 0.f, 0.f});
        for (size_t j = 0; j < m.size(); ++j) ev[i][j].mean = m[j];
        const int32_t K = read_len[i] - k + 1 > 0 ? read_len[i] - k + 1 : 0;
        std::vector<int32_t> s((size_t)K); rd(f, s.data(), s.size());
        map[i].resize((size_t)K);
        for (int32_t j = 0; j < K; ++j) map[i][(size_t)j] = abea_index_pair_t{s[(size_t)j], s[(size_t)j]};
        rd(f, &sc[i], 1); rd(f, &epb[i], 1);
    }
    fclose(f);
    abea_f5c_core core;
    memset(&core, 0, sizeof core);
    core.model = model.data(); core.kmer_size = (uint32_t)k; core.cuda_dev_id = 0; core.cuda_mem_frac = 0.1f;
    abea_f5c_init(&core);
    std::vector<char*> fasta(n);
    std::vector<const uint32_t*> cp(n);
    std::vector<abea_f5c_event_table> et(n);
    std::vector<abea_index_pair_t*> mp(n);
    for (int32_t i = 0; i < n; ++i) {
        fasta[i] = &seg[i][0]; cp[i] = cig[i].data(); mp[i] = map[i].empty() ? nullptr : map[i].data();
        et[i].n = ev[i].size(); et[i].start = 0; et[i].end = ev[i].size(); et[i].event = ev[i].data();
    }
    std::vector<int32_t> n_sites(n);
    std::vector<abea_meth_site_t*> sites(n);
    abea_f5c_meth_db db;
    memset(&db, 0, sizeof db);
    db.n_bam_rec = n; db.fasta_cache = fasta.data(); db.pos = pos.data(); db.cigar = cp.data(); db.n_cigar = n_cigar.data();
    db.is_rev = rev.data(); db.read_len = read_len.data(); db.et = et.data(); db.base_to_event_map = mp.data(); db.scalings = sc.data();
    db.events_per_base = epb.data(); db.read_stat_flag = flag.data(); db.cpgmodel = cpg.data(); db.n_sites = n_sites.data();
    db.sites = sites.data();
    abea_f5c_meth(&core, &db);
    std::string out = argv[2];
    FILE* o = fopen((out + ".sites").c_str(), "wb");
    for (int32_t i = 0; i < n; ++i) {
        fwrite(&n_sites[i], 4, 1, o);
        if (n_sites[i]) fwrite(sites[i], sizeof(abea_meth_site_t), (size_t)n_sites[i], o);
    }
    fclose(o);
    std::vector<const char*> contig(n, "ctg"), name(n);
    std::vector<std::string> names(n);
    for (int32_t i = 0; i < n; ++i) { names[i] = "read" + std::to_string(i); name[i] = names[i].c_str(); }
    std::vector<const abea_meth_site_t*> cs(sites.begin(), sites.end());
    const int64_t len = abea_meth_format_batch(nullptr, 0, 2, 1, n, contig.data(), name.data(), rev.data(), fasta.data(), pos.data(),
                                               flag.data(), n_sites.data(), cs.data(), (uint32_t)k, -1, -1, nullptr);
    if (len < 0) { fprintf(stderr, "abea_meth_format_batch: %lld\n", (long long)len); return 1; }
    std::string text((size_t)len + 1, '\0');
    abea_meth_format_batch(&text[0], text.size(), 2, 1, n, contig.data(), name.data(), rev.data(), fasta.data(), pos.data(), flag.data(),
                           n_sites.data(), cs.data(), (uint32_t)k, -1, -1, nullptr);
    o = fopen((out + ".tsv").c_str(), "wb");
    fwrite(text.data(), 1, (size_t)len, o);
    fclose(o);
    for (int32_t i = 0; i < n; ++i) free(sites[i]);
    printf("meth_driver: %d reads, meth_time %.6f s\n", n, db.meth_time);
    abea_f5c_free(&core);
    return 0;
}
