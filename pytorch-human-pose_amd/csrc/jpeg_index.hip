// The index of a restart-less JPEG stream built on the GPU, with no Huffman pass on the host (the rule and its invariants are stated at
// hh_jpeg_index_device_batch in include/hhrnet.h; the arithmetic, jpeg_idx_walk included, is jpeg_dec_math.h, shared with the host twin
// jpeg_idx_sync_host).
//
// jpeg_index_kernel: one workgroup of 1024 lanes per image; an image with DRI, or whose table block does not ask for it, ends the
// workgroup at once.  The image's eight Huffman tables are copied to LDS, as in jpeg_dec_entropy_kernel.  A round takes the next 1024
// subsequences of the scan, lane t the t-th: it walks whole blocks from its start state (lane 0: the verified end of the round before,
// the others a guess) to its first boundary in the next subsequence and leaves that exit state in LDS.  The passes that follow hand
// exit states down the line until no lane's start differs from its predecessor's exit; what a lane keeps (start state, block count,
// DC sums) stays in its registers.  The block counts and DC sums are then scanned (inclusive scans inside each wave by shuffles, the 16
// wave totals through LDS), and the lanes up to the first one without an exit walk once more from their verified states and write the
// entries whose MCU boundary they cross.  The round's last exit, the block total and the DC totals start the next round.
//
// Every wait is a barrier of this one workgroup, reached by all 1024 lanes: the loop bounds (rounds, passes) and every condition
// around a barrier are computed from LDS words or kernel arguments and are the same in all lanes.  Entries are written as whole 32-byte
// structs (vector stores).
#include "kernels.h"
#include "jpeg_dec_math.h"

// The inclusive scan of v over the workgroup's lanes -> this lane's exclusive prefix; *all: the workgroup's total.  part: 16 words of
// LDS per call site (a barrier separates its write from its reads; the caller's next barrier protects its reuse).
template <class T>
__device__ __forceinline__ T jpeg_idx_scan(T v, T *part, T *all)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    if (lane == 63) part[wave] = incl;
    __syncthreads();
    T before = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < JPEG_IDX_LANES / 64; ++w) {
        const T p = part[w];
        before += w < wave ? p : 0;
        sum += p;
    }
    *all = sum;
    return before + incl - v;
}

__global__ __launch_bounds__(JPEG_IDX_LANES) void jpeg_index_kernel(unsigned char *__restrict__ base, const JpegDecDesc *__restrict__ descs, int mps, int B,
                                                                    int32_t *__restrict__ status)
{
    __shared__ JpegHuff huff[8];
    __shared__ JpegIdxKey exits[JPEG_IDX_LANES];
    __shared__ unsigned long long part_g[JPEG_IDX_LANES / 64];
    __shared__ uint32_t part_dc[3][JPEG_IDX_LANES / 64];
    __shared__ int first_bad;
    const JpegDecDesc d = descs[blockIdx.x];
    unsigned char *tab = base + d.tables_offset;
    const JpegStreamInfo I = *reinterpret_cast<const JpegStreamInfo *>(tab);
    if (I.restart_interval || I.reserved[1] != JPEG_IDX_PENDING) return;  // (the whole workgroup)
    const uint32_t *src = reinterpret_cast<const uint32_t *>(tab + JPEG_DEC_TABLES_AT + offsetof(JpegDecTables, huff));
    for (int i = threadIdx.x; i < (int)(sizeof(huff) / 4); i += JPEG_IDX_LANES) reinterpret_cast<uint32_t *>(huff)[i] = src[i];
    const int t = threadIdx.x;
    const unsigned char *b = base + d.stream_offset;
    const int E = jpeg_idx_scan_end(I, d.stream_length);
    const long long nsub = jpeg_idx_subsequences(I, d.stream_length, B), total = (long long)I.mcols * I.mrows * I.bpm;
    JpegSegment *seg = reinterpret_cast<JpegSegment *>(tab + JPEG_DEC_SEGS_AT);
    // what a round hands to the next: the same in every lane
    JpegIdxKey carry = jpeg_idx_key((int)I.scan_offset, 0, 0);
    unsigned long long g = 0;
    uint32_t dc[3] = {0, 0, 0};
#pragma unroll 1
    for (long long k0 = 0; k0 < nsub && g < (unsigned long long)total && carry != JPEG_IDX_NONE; k0 += JPEG_IDX_LANES) {
        const int n = (int)(nsub - k0 < JPEG_IDX_LANES ? nsub - k0 : JPEG_IDX_LANES);
        const bool active = t < n;
        const int limit = jpeg_idx_limit(I, nsub, k0 + t, B);
        JpegIdxKey start = JPEG_IDX_NONE;
        JpegIdxLane mine;
        mine.exit = JPEG_IDX_NONE, mine.count = 0, mine.dc[0] = mine.dc[1] = mine.dc[2] = 0, mine.status = 0;
        __syncthreads();  // the tables are in LDS; the round before has read exits[] and first_bad
        if (t == 0) first_bad = n;  // (the first barrier of the passes below stands between this and the atomicMin)
        if (active) {
            start = t == 0 ? carry : jpeg_idx_guess(b, I, k0 + t, B);
            jpeg_idx_walk<false>(b, E, I, huff, start, limit, 0, total, mps, nullptr, nullptr, 0, mine);
        }
        exits[t] = mine.exit;
        // lane 0 is true, so after k passes lanes 0..k are: at most n passes
#pragma unroll 1
        for (int it = 0; it < n; ++it) {
            __syncthreads();  // every exit of the pass before is in LDS
            bool redo = false;
            if (active && t > 0) {
                const JpegIdxKey prev = exits[t - 1];
                if (prev != JPEG_IDX_NONE && prev != start) start = prev, redo = true;
            }
            if (!__syncthreads_or(redo)) break;  // (a barrier: every lane has read its predecessor's exit)
            if (redo) {
                jpeg_idx_walk<false>(b, E, I, huff, start, limit, 0, total, mps, nullptr, nullptr, 0, mine);
                exits[t] = mine.exit;
            }
        }
        if (active && mine.exit == JPEG_IDX_NONE) atomicMin(&first_bad, t);
        unsigned long long sum_g;
        uint32_t sum_dc[3], pre_dc[3];
        const unsigned long long pre_g = g + jpeg_idx_scan<unsigned long long>(mine.count, part_g, &sum_g);
#pragma unroll
        for (int c = 0; c < 3; ++c) pre_dc[c] = dc[c] + jpeg_idx_scan<uint32_t>(mine.dc[c], part_dc[c], &sum_dc[c]);
        __syncthreads();  // first_bad is final
        const int bad = first_bad;
        const JpegIdxKey last_exit = exits[n - 1];
        if (active && t <= bad && pre_g < (unsigned long long)total) {
            JpegIdxLane last;
            jpeg_idx_walk<true>(b, E, I, huff, start, limit, (long long)pre_g, total, mps, pre_dc, seg, d.nseg, last);
            if (last.status) {
                atomicMax(status + blockIdx.x, last.status);
                reinterpret_cast<JpegStreamInfo *>(tab)->reserved[0] = last.status;  // the decode's entropy launch skips this image
            }
        }
        g += sum_g, dc[0] += sum_dc[0], dc[1] += sum_dc[1], dc[2] += sum_dc[2];
        carry = bad < n ? JPEG_IDX_NONE : last_exit;
    }
}

hipError_t launch_jpeg_index(unsigned char *base, const hh_jpeg_dec_desc *descs, int n, int mps, int subseq_bytes, int32_t *status, hipStream_t s)
{
    hipLaunchKernelGGL(jpeg_index_kernel, dim3(n), dim3(JPEG_IDX_LANES), 0, s, base, descs, mps, subseq_bytes, status);
    return hipGetLastError();
}
