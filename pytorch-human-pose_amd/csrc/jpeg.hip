// Baseline JPEG on the GPU for a batch of frames of mixed sizes, qualities and subsamplings: three launches per call, whatever the
// batch.  The rule is stated at hh_jpeg_encode_u8_batch in include/hhrnet.h; its arithmetic is jpeg_math.h, shared with the host.
//
// jpeg_transform_kernel: a wave owns one MCU, a workgroup JPEG_MCUS_PER_GROUP = 4 of them.  Every lane converts its pixels (one in
// 4:4:4, a 2 x 2 group with its chroma mean in 4:2:0) into LDS; lanes 0 .. 8 * blocks - 1 then own one row of one block for the row
// pass and one column for the column pass and the quantiser, which scatters into the block's zigzag order in LDS; the same lanes store
// 8 coefficients each as one 16-byte vector.  The two quantisation tables of the frame's quality are formed in LDS by the workgroup.
//
// jpeg_entropy_kernel: one wave per restart interval (one MCU row).  JPEG_ENT_LANES = 64 blocks per pass: a lane walks its block once
// to count its bits, a wave scan turns the counts into bit offsets behind the partial byte carried over from the pass before, the lane
// walks the block again and ORs its codes into the LDS bit buffer (LDS atomics: two lanes may share a word), then the finished bytes
// leave four to a lane: a second scan over the lanes' byte counts with their FF 00 pairs gives every lane its place in the interval's
// slot of the workspace.  The buffer holds the worst case of 64 blocks (JPEG_BLOCK_BITS each), the slot the worst case of the
// interval (jpeg_interval_bound): no length is assumed "typical".
//
// jpeg_pack_kernel: workgroup r of a frame sums the interval lengths before r, copies interval r to its final place and appends its
// RSTm; the workgroup behind the last interval writes the header, EOI and lengths[frame].
#include "kernels.h"
#include "jpeg_math.h"

__global__ __launch_bounds__(64 * JPEG_MCUS_PER_GROUP) void jpeg_transform_kernel(const unsigned char *__restrict__ base, unsigned char *__restrict__ ws,
                                                                                  const JpegDesc *__restrict__ descs)
{
    __shared__ int32_t smp[JPEG_MCUS_PER_GROUP][6 * 64];
    __shared__ __attribute__((aligned(16))) int16_t zz[JPEG_MCUS_PER_GROUP][6 * 64];
    __shared__ uint16_t Q[2][64];
    const JpegDesc d = descs[blockIdx.z];
    const JpegGeom g = jpeg_geom(d.h, d.w, d.subsampling);
    const int nmcu = g.mrows * g.mcols;  // <= 8192 * 8192
    if ((int)blockIdx.x * JPEG_MCUS_PER_GROUP >= nmcu) return;  // (the whole workgroup: the grid is sized for the largest frame)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mcu = (int)blockIdx.x * JPEG_MCUS_PER_GROUP + wave;
    const bool active = mcu < nmcu;
    if (tid < 128) Q[tid >> 6][tid & 63] = (uint16_t)jpeg_quant(d.quality, tid >> 6, tid & 63);
    if (active) jpeg_mcu_samples(base + d.src_offset, d, mcu / g.mcols, mcu % g.mcols, lane, smp[wave]);
    __syncthreads();
    const bool owner = active && lane < g.bpm * 8;  // a row, then a column, then 8 coefficients of block lane / 8
    if (owner) jpeg_fdct_row(smp[wave] + lane * 8);
    __syncthreads();
    if (owner) jpeg_fdct_col_quant(smp[wave] + (lane >> 3) * 64, lane & 7, Q[jpeg_block_is_luma(lane >> 3, g.bpm) ? 0 : 1], zz[wave] + (lane >> 3) * 64);
    __syncthreads();
    if (owner) {
        // block mcu * bpm + lane / 8 of the frame's mrows * nblk blocks: inside coef_bytes
        JpegVec8 *out = reinterpret_cast<JpegVec8 *>(ws + d.ws_offset) + (size_t)mcu * g.bpm * 8 + lane;
        *out = *reinterpret_cast<const JpegVec8 *>(zz[wave] + lane * 8);
    }
}

__device__ __forceinline__ int jpeg_wave_scan(int v, int lane)  // inclusive, over the 64 lanes
{
#pragma unroll
    for (int delta = 1; delta < 64; delta <<= 1) {
        const int t = __shfl_up(v, delta, 64);
        if (lane >= delta) v += t;
    }
    return v;
}

// Bits into the LDS buffer at bit position pos, most significant bit first within a word.
struct JpegLdsSink {
    uint32_t *words;
    uint32_t pos;
    __device__ __forceinline__ void put(uint32_t bits, int count)  // 1 <= count <= 26
    {
        const uint32_t sh = pos & 31u, w = pos >> 5;
        const uint64_t v = (uint64_t)bits << (64u - (uint32_t)count - sh);
        atomicOr(&words[w], (uint32_t)(v >> 32));
        if (sh + (uint32_t)count > 32u) atomicOr(&words[w + 1], (uint32_t)v);  // (bits of this block: below the pass's total)
        pos += (uint32_t)count;
    }
};

__global__ __launch_bounds__(JPEG_ENT_LANES) void jpeg_entropy_kernel(unsigned char *__restrict__ ws, const JpegDesc *__restrict__ descs)
{
    __shared__ uint32_t words[JPEG_ENT_WORDS];
    __shared__ JpegCodes codes;
    const JpegDesc d = descs[blockIdx.z];
    const JpegGeom g = jpeg_geom(d.h, d.w, d.subsampling);
    const int row = blockIdx.x, lane = threadIdx.x;
    if (row >= g.mrows) return;  // (the whole workgroup)
    for (int i = lane; i < (int)(sizeof(JpegCodes) / 4); i += JPEG_ENT_LANES) reinterpret_cast<uint32_t *>(&codes)[i] = 0;
    __syncthreads();
    if (lane < 4) jpeg_build_table(&codes, lane);
    __syncthreads();

    unsigned char *frame_ws = ws + d.ws_offset;
    const int16_t *coefs = reinterpret_cast<const int16_t *>(frame_ws) + (size_t)row * g.nblk * 64;
    unsigned char *slot = frame_ws + g.coef_bytes + (size_t)row * g.slot;
    uint32_t carry_bits = 0, carry_byte = 0;  // the pass before left carry_bits < 8 bits, at the top of carry_byte
    uint32_t outpos = 0;                      // bytes of the slot written so far: <= 2 * (bytes of all bits so far) <= jpeg_interval_bound

    for (int first = 0; first < g.nblk; first += JPEG_ENT_LANES) {  // (uniform over the wave)
        const int j = first + lane;
        const bool have = j < g.nblk;
        const int t = jpeg_block_is_luma(j, g.bpm) ? 0 : 1;
        int pred = 0, bits = 0;
        if (have) {
            const int pj = jpeg_pred_block(j, g.bpm);
            if (pj >= 0) pred = coefs[(size_t)pj * 64];
            JpegCountSink count = {0};
            jpeg_code_block(coefs + (size_t)j * 64, pred, codes.dc[t], codes.ac[t], count);
            bits = count.bits;  // <= JPEG_BLOCK_BITS
        }
        const int incl = jpeg_wave_scan(bits, lane);
        const uint32_t total = carry_bits + (uint32_t)__shfl(incl, 63, 64);  // <= 7 + 64 * JPEG_BLOCK_BITS: inside `words`
        const uint32_t nwords = (total + 31u) >> 5;
        for (uint32_t i = lane; i < nwords; i += JPEG_ENT_LANES) words[i] = i == 0 ? carry_byte << 24 : 0u;
        __syncthreads();
        if (have) {
            JpegLdsSink sink = {words, carry_bits + (uint32_t)(incl - bits)};
            jpeg_code_block(coefs + (size_t)j * 64, pred, codes.dc[t], codes.ac[t], sink);
        }
        __syncthreads();

        const bool last = first + JPEG_ENT_LANES >= g.nblk;
        uint32_t nbytes = total >> 3, rest = total & 7u;
        const uint32_t tail = total >> 3;  // the byte that holds the `rest` bits
        const bool pad = last && rest != 0;
        if (pad) nbytes += 1;  // the interval's last byte, filled up with 1-bits below
        for (uint32_t b0 = 0; b0 < nbytes; b0 += 4 * JPEG_ENT_LANES) {  // (uniform)
            const uint32_t k = b0 + 4u * lane;
            uint32_t wv = k < nbytes ? words[k >> 2] : 0u;  // k >> 2 < nwords
            if (pad && (tail >> 2) == (k >> 2)) wv |= (0xffu >> rest) << (24u - 8u * (tail & 3u));
            const int mine = k < nbytes ? (int)min(4u, nbytes - k) : 0;
            int nout = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < mine) nout += ((wv >> (24 - 8 * e)) & 255u) == 255u ? 2 : 1;
            const int incl2 = jpeg_wave_scan(nout, lane);
            uint32_t at = outpos + (uint32_t)(incl2 - nout);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < mine) {
                    const uint32_t b = (wv >> (24 - 8 * e)) & 255u;
                    slot[at++] = (unsigned char)b;
                    if (b == 255u) slot[at++] = 0;
                }
            outpos += (uint32_t)__shfl(incl2, 63, 64);
        }
        carry_bits = pad ? 0u : rest;
        carry_byte = carry_bits ? (words[tail >> 2] >> (24u - 8u * (tail & 3u))) & 255u : 0u;
        __syncthreads();  // the next pass clears the buffer
    }
    if (lane == 0) reinterpret_cast<int32_t *>(frame_ws + g.coef_bytes + (size_t)g.mrows * g.slot)[row] = (int32_t)outpos;
}

#define JPEG_PACK_THREADS 256
__global__ __launch_bounds__(JPEG_PACK_THREADS) void jpeg_pack_kernel(unsigned char *__restrict__ base, const unsigned char *__restrict__ ws,
                                                                      const JpegDesc *__restrict__ descs, int32_t *__restrict__ lengths)
{
    __shared__ long long part[JPEG_PACK_THREADS];
    const JpegDesc d = descs[blockIdx.z];
    const JpegGeom g = jpeg_geom(d.h, d.w, d.subsampling);
    const int r = blockIdx.x, tid = threadIdx.x;
    if (r > g.mrows) return;  // (the whole workgroup)
    const unsigned char *frame_ws = ws + d.ws_offset;
    const int32_t *lens = reinterpret_cast<const int32_t *>(frame_ws + g.coef_bytes + (size_t)g.mrows * g.slot);
    long long sum = 0;
    for (int i = tid; i < r; i += JPEG_PACK_THREADS) sum += lens[i];  // r <= mrows
    part[tid] = sum;
    __syncthreads();
    for (int s = JPEG_PACK_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) part[tid] += part[tid + s];
        __syncthreads();
    }
    // the bytes in front of interval r: header, the intervals before it, a marker behind each of those.  With every length at most its
    // bound the stream ends at or below jpeg_bound <= out_capacity (checked on the host).
    const long long at = JPEG_HEADER_BYTES + part[0] + 2ll * r;
    unsigned char *out = base + d.out_offset;
    if (r < g.mrows) {
        const unsigned char *slot = frame_ws + g.coef_bytes + (size_t)r * g.slot;
        const int len = lens[r];
        for (int i = tid; i < len; i += JPEG_PACK_THREADS) out[at + i] = slot[i];
        if (tid == 0) {
            out[at + len] = 0xff;
            out[at + len + 1] = (unsigned char)(r + 1 < g.mrows ? 0xd0 + (r & 7) : 0xd9);
        }
    } else if (tid == 0) {
        jpeg_write_header(out, d.h, d.w, d.subsampling, d.quality, g.mcols);
        lengths[blockIdx.z] = (int32_t)at;  // (at counts the marker behind the last interval: EOI)
    }
}

hipError_t launch_jpeg_encode(unsigned char *base, const JpegDesc *descs, int n, int max_mcus, int max_rows, unsigned char *ws, int32_t *lengths,
                              hipStream_t s)
{
    hipLaunchKernelGGL(jpeg_transform_kernel, dim3((max_mcus + JPEG_MCUS_PER_GROUP - 1) / JPEG_MCUS_PER_GROUP, 1, n), dim3(64 * JPEG_MCUS_PER_GROUP), 0, s,
                       base, ws, descs);
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(max_rows, 1, n), dim3(JPEG_ENT_LANES), 0, s, ws, descs);
    hipLaunchKernelGGL(jpeg_pack_kernel, dim3(max_rows + 1, 1, n), dim3(JPEG_PACK_THREADS), 0, s, base, ws, descs, lengths);
    return hipGetLastError();
}
