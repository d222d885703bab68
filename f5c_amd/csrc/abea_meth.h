/* abea_meth.h — device records of the call-methylation job builder (abea_meth.hip), shared with its host driver (abea_meth.cpp). */
#ifndef ABEA_METH_H
#define ABEA_METH_H
#include <stdint.h>
#include "../../include/abea.h"

#define ABEA_METH_SEP      10     /* min_separation, meth.c:495 */
#define ABEA_METH_MAX_SPAN 200    /* meth.c:521 */
#define ABEA_METH_SEQ_SLOT 224    /* bytes per emitted sequence: a surviving group's subseq has at most 200 + 21 bases + NUL */

/* one read of a launch; offsets into the launch's flattened arrays */
typedef struct __attribute__((aligned(16))) {
    int64_t seg_off;       /* bytes of the reference segment (db->fasta_cache[i]) */
    int64_t cigar_off;     /* uint32 CIGAR words */
    int64_t map_off;       /* int32: base_to_event_map[i][j].start */
    int64_t scratch_off;   /* int32 words: CpG positions (seg_len / 2 + 1), then the event-alignment record (2 * read_len) */
    int64_t group_off;     /* emit pass: first group record / sequence slot pair of the read */
    int32_t seg_len, read_len, n_cigar, n_events;
    int32_t pos, rc, pad0, pad1;
} abea_meth_read;

/* one surviving CpG group: the arguments of its two profile_hmm_score calls (meth.c:555-570) and its ScoredSite (:575-598).
 * Its sequences sit at seqs + 2 * ABEA_METH_SEQ_SLOT * g (unmethylated, then methylated; reverse-complemented on a reverse read) */
typedef struct {
    int32_t e1, e2;                       /* event_start_idx, event_stop_idx; stride = e1 <= e2 ? 1 : -1 */
    int32_t start, end, n_cpg;            /* start_position, end_position (reference coordinates), n_cpg */
    int32_t seq_len;
    int32_t pad0, pad1;
} abea_meth_group;

/* per read, written by both passes */
typedef struct { int32_t n_groups; int32_t n_skipped; int32_t error; int32_t pad; } abea_meth_count;

#define ABEA_METH_ERR_CIGAR 1     /* N (ref skip) or an op get_aligned_segments does not handle (meth.c:60-73) */
#define ABEA_METH_ERR_BASE  2     /* a segment byte that is no IUPAC code (meth.c:302: assert(isValid)) */

#endif
