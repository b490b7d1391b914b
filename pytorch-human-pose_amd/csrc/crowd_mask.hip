// Crowd masks filled on the GPU from toggle lists (the rule is stated at hh_crowd_masks_u8_batch in include/hhrnet.h): all masks of a
// batch, of mixed sizes, in ONE launch.  The work is a transposition: toggles are ordered column-major (idx = x * h + y), the output
// is row-major bytes.
//
// A workgroup owns a tile of CROWD_TW = 256 columns x CROWD_TH = 32 rows (crowd_mask_math.h).  Phase 1: lane l owns column l of the
// tile; per segment that its column range does not cull it does one upper-bound search for the tile's top row and walks down with a
// cursor, and it ORs the coverage over the segments into one uint32 (bit r = row r).  The 256 words go to LDS as consecutive dwords
// (conflict-free under the 32-bank rule of ds_write_b32: the 32 lanes of a half-wave hit 32 different banks).  Phase 2: a wave owns
// a row of the tile at a time, lane g the four bytes of one 4-byte-aligned dword of that row in memory.  Mask offsets and widths carry
// no alignment guarantee, so per row `head` = the 0..3 bytes in front of the first aligned dword is taken from the row's address;
// the head bytes and a ragged tail are stored as bytes, everything between as whole dwords (a wave stores 256 contiguous bytes).
// Each lane reads its eight candidate words from LDS once (two aligned ds_read_b128, consecutive lanes on consecutive 16-byte
// slots) and picks four per row by `head`, which is uniform over the wave.  Every mask byte is written exactly once by exactly one
// lane; no atomics; nothing depends on the launch.
#include "kernels.h"
#include "crowd_mask_math.h"

__global__ __launch_bounds__(CROWD_THREADS) void crowd_masks_kernel(unsigned char *base, const CrowdMaskDesc *__restrict__ descs,
                                                                    const CrowdSegDesc *__restrict__ segs)
{
    __shared__ __attribute__((aligned(16))) uint32_t colbits[CROWD_TW + 4];  // + one group of zeros that the last lane's second read meets
    const CrowdMaskDesc d = descs[blockIdx.y];
    const int xtiles = (d.w + CROWD_TW - 1) / CROWD_TW, ytiles = (d.h + CROWD_TH - 1) / CROWD_TH;
    if ((int)blockIdx.x >= xtiles * ytiles) return;  // the grid is sized for the largest mask; uniform over the workgroup
    const int tx0 = ((int)blockIdx.x % xtiles) * CROWD_TW, ty0 = ((int)blockIdx.x / xtiles) * CROWD_TH;
    const int rows = d.h - ty0 < CROWD_TH ? d.h - ty0 : CROWD_TH, cols = d.w - tx0 < CROWD_TW ? d.w - tx0 : CROWD_TW;
    const int lane = threadIdx.x;

    colbits[lane] = lane < cols ? crowd_lane_bits(base, segs, d, tx0 + lane, ty0, rows) : 0u;
    if (lane < 4) colbits[CROWD_TW + lane] = 0u;
    __syncthreads();

    const int g = lane % 64;  // the dword group within a row
    uint32_t W[8];
    {
        const uint4 a = *reinterpret_cast<const uint4 *>(&colbits[4 * g]), b = *reinterpret_cast<const uint4 *>(&colbits[4 * g + 4]);
        W[0] = a.x, W[1] = a.y, W[2] = a.z, W[3] = a.w, W[4] = b.x, W[5] = b.y, W[6] = b.z, W[7] = b.w;
    }
    unsigned char *tile = base + d.mask_offset + (size_t)ty0 * d.w + tx0;  // inside the mask: ty0 < h, tx0 < w
    for (int r = lane / 64; r < rows; r += CROWD_THREADS / 64) {
        unsigned char *row = tile + (size_t)r * d.w;
        const int head = (int)((4 - (reinterpret_cast<uintptr_t>(row) & 3)) & 3);
        if (g < head && g < cols) row[g] = (colbits[g] >> r & 1) ? 0 : 255;
        const int c = head + 4 * g;  // the tile column of this lane's dword; columns from `cols` on are not this tile's
        if (c >= cols) continue;
        uint32_t v0, v1, v2, v3;
        switch (head) {
        case 0: v0 = W[0], v1 = W[1], v2 = W[2], v3 = W[3]; break;
        case 1: v0 = W[1], v1 = W[2], v2 = W[3], v3 = W[4]; break;
        case 2: v0 = W[2], v1 = W[3], v2 = W[4], v3 = W[5]; break;
        default: v0 = W[3], v1 = W[4], v2 = W[5], v3 = W[6]; break;
        }
        // a covered pixel (bit set) is byte 0, every other 255
        const uint32_t word = (((v0 >> r & 1) - 1) & 0xffu) | (((v1 >> r & 1) - 1) & 0xffu) << 8 | (((v2 >> r & 1) - 1) & 0xffu) << 16 | (((v3 >> r & 1) - 1) & 0xffu) << 24;
        if (c + 3 < cols) {
            *reinterpret_cast<uint32_t *>(row + c) = word;  // 4-byte aligned by the choice of head
        } else {
            for (int e = 0; c + e < cols; ++e) row[c + e] = (unsigned char)(word >> (8 * e));
        }
    }
}

hipError_t launch_crowd_masks(unsigned char *base, const CrowdMaskDesc *descs, const CrowdSegDesc *segs, int n, int max_tiles, hipStream_t s)
{
    hipLaunchKernelGGL(crowd_masks_kernel, dim3(max_tiles, n), dim3(CROWD_THREADS), 0, s, base, descs, segs);
    return hipGetLastError();
}
