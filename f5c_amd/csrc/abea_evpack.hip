/* abea_evpack.hip — the narrower event-table records of the raw-signal host entries (abea_*_batch_host_fields, include/abea.h).
 *
 * abea_ev_pack_kernel (abea_kernels.hip) packs a chunk's tables into 12-byte {u32 start, f32 mean, f32 stdv} records for
 * ABEA_EV_FIELDS_ALL.  A caller that reads fewer fields of each event asks for a narrower record, and only those bytes cross PCIe:
 *   ABEA_EV_FIELDS_NO_STDV  {u32 start, f32 mean}   8 B per event   (call-methylation: the profile HMM reads the means, hmm.c:85)
 *   ABEA_EV_FIELDS_LAYOUT   {u32 start}             4 B per event   (resquiggle: output_db_rsq reads start / length)
 * `length` is rebuilt on the host from the neighbour's start, as for the 12-byte form (abea_chain.cpp: unpack_events).
 * Same scheme as the 12-byte kernel: block = read, a thread packs 4 consecutive events into W 16-byte stores (W = words per
 * record), so the lanes of a wavefront store 64 x 16W contiguous bytes; dst_ptr counts records and is a multiple of 4 per read,
 * and the records past a read's last event up to that multiple are written as zero. */
#include <hip/hip_runtime.h>
#include "abea_device.h"

template <int W>
static __device__ __forceinline__ void ev_pack_narrow(int n_reads, const abea_event_t* __restrict__ src, const int64_t* __restrict__ src_ptr,
                                                      const int64_t* __restrict__ dst_ptr, const int32_t* __restrict__ n_events,
                                                      uint4* __restrict__ dst) {
    static_assert(W == 1 || W == 2, "narrow records: start, or start + mean");
    const int r = blockIdx.x;
    if (r >= n_reads) return;
    const abea_event_t* __restrict__ s = src + src_ptr[r];
    uint4* __restrict__ d = dst + dst_ptr[r] / 4 * W;
    const int ne = max(n_events[r], 0);
    for (int g = threadIdx.x; g * 4 < ne; g += blockDim.x) {
        uint32_t w[4 * W];
        #pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = g * 4 + i;
            const bool in = j < ne;
            w[W * i] = in ? (uint32_t)s[j].start : 0u;
            if (W == 2) w[W * i + 1] = in ? __float_as_uint(s[j].mean) : 0u;
        }
        #pragma unroll
        for (int q = 0; q < W; ++q) d[(size_t)g * W + q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
    }
}

/* ABEA_EV_FIELDS_NO_STDV: {u32 start, f32 mean}, two 16-byte stores per 4 events */
extern "C" __global__ __launch_bounds__(256)
void abea_ev_pack8_kernel(int n_reads, const abea_event_t* __restrict__ src, const int64_t* __restrict__ src_ptr,
                          const int64_t* __restrict__ dst_ptr, const int32_t* __restrict__ n_events, uint4* __restrict__ dst) {
    ev_pack_narrow<2>(n_reads, src, src_ptr, dst_ptr, n_events, dst);
}

/* ABEA_EV_FIELDS_LAYOUT: {u32 start}, one 16-byte store per 4 events */
extern "C" __global__ __launch_bounds__(256)
void abea_ev_pack4_kernel(int n_reads, const abea_event_t* __restrict__ src, const int64_t* __restrict__ src_ptr,
                          const int64_t* __restrict__ dst_ptr, const int32_t* __restrict__ n_events, uint4* __restrict__ dst) {
    ev_pack_narrow<1>(n_reads, src, src_ptr, dst_ptr, n_events, dst);
}
