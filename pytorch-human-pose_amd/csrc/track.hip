// Pose tracking across video frames on the GPU: ids and One-Euro smoothing behind hh_decode (the rule is stated at hh_track_step in
// include/hhrnet.h; the arithmetic and the bookkeeping of one slot / one joint are track_math.h, shared with the host).
//
// track_kernel: grid (S), one workgroup of TRACK_THREADS = 256 threads per stream, which walks its F frames in order.  Latency work: a few
// dozen tracks times a few dozen detections per frame, so the layout serves short dependent phases, not throughput.
//   The stream's state is copied into LDS once, used there for all F frames and copied back once, when it fits next to the similarity
//   matrix (T * P fp64); otherwise the same code works on the global copy through the same (flat) pointers: identical results.
//   Per frame, five phases with a barrier behind each:
//   0. all threads: x, y, score of the frame's P * K joints from global memory into LDS, coalesced (one round trip for the frame; every
//      later phase reads the rows from there, the tags are never read).
//   1. wave 0, lane d: is row d a valid detection?  The rows become one 64-bit set (ballot).
//   2. all threads: the T x P similarities into LDS, one pair per thread per step.
//   3. wave 0, lane t = slot t: greedy assignment.  Per round every unmatched live lane scans its row for its best free detection, a
//      butterfly of shuffles finds the best candidate of the wave (comparisons only), its lane takes it; a lane scans its row again only
//      after its candidate's detection was taken.  At most min(T, P) rounds.  Then
//      the same lanes free, match or open their slots (free slots and unmatched rows are two ballots; the j-th free slot takes the j-th
//      unmatched row) and leave per slot: row, id, fresh, Te, alpha(d_cutoff).
//   4. all threads: one (row, joint) per thread per step: the filter, the slot's raw pose, the row's smooth pair; lane d: the row's id.
//   Every output element of the S * F frames is written exactly once, unconditionally; no atomics, no spin-waits, nothing crosses
//   workgroups, and nothing but the state carries over between calls.
#include "kernels.h"
#include "track_math.h"

enum { TRACK_MODE_STEP = 0, TRACK_MODE_SIM = 1 };
enum { TRACK_LDS_BUDGET = 156 * 1024 };  // of the CU's 160 KB: the static arrays below need ~2 KB

// Step 3 by one wave: lane t holds row t (id == 0: no live track); returns the lane's detection or -1, *taken = the matched rows.
__device__ __forceinline__ int track_wave_assign(const double *sim, int t, int P, int id, double min_oks, uint64_t *taken_out)
{
    int my = -1, row_d = -2;  // row_d: the row's best free detection, -1 = none is left, -2 = scan the row
    double row_s = 0.0;
    uint64_t taken = 0;
    for (;;) {
        if (id != 0 && my < 0 && row_d == -2) row_d = track_row_best(sim + (size_t)t * P, P, taken, min_oks, &row_s);
        double cs = row_s;
        int cd = id != 0 && my < 0 ? row_d : -1, cid = id;
        for (int o = 32; o; o >>= 1) {
            const double os = __shfl_xor(cs, o);
            const int oid = __shfl_xor(cid, o), od = __shfl_xor(cd, o);
            if (track_better(os, oid, od, cs, cid, cd)) { cs = os; cid = oid; cd = od; }
        }
        if (cd < 0) break;  // (the same on all lanes: live ids are distinct, so the butterfly has one winner)
        if (id != 0 && id == cid) my = cd;
        if (row_d == cd) row_d = -2;  // (taken only grows: a candidate that is still free is still the row's best)
        taken |= (uint64_t)1 << cd;
    }
    *taken_out = taken;
    return my;
}

__global__ __launch_bounds__(TRACK_THREADS) void track_kernel(const TrackParams p, unsigned char *state_all, long long state_stride,
                                                              const float *__restrict__ joints, const float *__restrict__ scores,
                                                              const int32_t *__restrict__ num_people, const int32_t *__restrict__ flags, int F, int mode,
                                                              int lds_state, int32_t *__restrict__ track_ids, float *__restrict__ smooth,
                                                              int32_t *__restrict__ out_flags, double *__restrict__ sim_out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ double s_te[HH_TRACK_MAX_TRACKS], s_ad[HH_TRACK_MAX_TRACKS];
    __shared__ uint64_t s_valid;
    __shared__ int s_det_slot[HH_TRACK_MAX_PEOPLE], s_slot_id[HH_TRACK_MAX_TRACKS];
    __shared__ unsigned char s_fresh[HH_TRACK_MAX_TRACKS];
    const int tid = threadIdx.x, s = blockIdx.x;  // s < S = the grid's size
    const int T = p.max_tracks, P = p.max_people, K = p.K, W = 3 + p.E;
    double *s_sim = reinterpret_cast<double *>(smem);  // [T, P]
    unsigned char *home = state_all + (size_t)s * state_stride;
    const int words = (int)(track_state_bytes(K, T) / 8);
    float *s_det = reinterpret_cast<float *>(smem + (size_t)T * P * 8);  // [P, K, 3] x, y, score of the frame
    unsigned char *base = lds_state ? smem + (((size_t)T * P * 8 + (size_t)P * K * 12 + 7) & ~(size_t)7) : home;
    if (lds_state) {
        for (int i = tid; i < words; i += TRACK_THREADS) reinterpret_cast<uint64_t *>(base)[i] = reinterpret_cast<const uint64_t *>(home)[i];
        __syncthreads();
    }
    const TrackState st = track_state_view(base, K, T);
    for (int f = 0; f < F; ++f) {
        const size_t b = (size_t)s * F + f;  // b < S * F = B
        const float *jb = joints + b * P * K * W;
        const int n = num_people[b], fl = flags ? flags[b] : 0;
        const int issued = st.hdr[0];
        for (int e = tid; e < P * K * 3; e += TRACK_THREADS) s_det[e] = jb[(size_t)(e / 3) * W + e % 3];  // e / 3 < P * K
        __syncthreads();
        if (tid < 64) {
            bool v = false;
            if (tid < P && tid < n && !(fl & (HH_DECODE_FALLBACK | HH_DECODE_SOLVER_GUARD))) v = track_det_valid(s_det + (size_t)tid * K * 3, 3, scores[b * P + tid], p);
            const uint64_t m = __ballot(v);
            if (tid == 0) s_valid = m;
            s_det_slot[tid] = -1;
        }
        __syncthreads();
        const uint64_t valid = s_valid;
        for (int pair = tid; pair < T * P; pair += TRACK_THREADS) {
            const int t = pair / P, d = pair % P;
            double v = 0.0;
            if (st.id[t] != 0 && ((valid >> d) & 1)) v = track_similarity(st.xy + (size_t)t * K * 2, st.score + (size_t)t * K, st.area[t], s_det + (size_t)d * K * 3, 3, p);
            if (mode == TRACK_MODE_SIM) sim_out[(size_t)s * T * P + pair] = v;  // (F == 1)
            else s_sim[pair] = v;
        }
        if (mode == TRACK_MODE_SIM) return;
        __syncthreads();
        if (tid < 64) {
            const int t = tid;
            const bool slot = t < T;
            uint64_t taken;
            const int my = track_wave_assign(s_sim, t, P, slot ? st.id[t] : 0, p.min_oks, &taken);
            const uint64_t free_set = __ballot(slot && track_slot_free(st, t, my, p));
            const uint64_t unmatched = valid & ~taken;
            bool fresh = false;
            double Te = 0.0;
            int det = -1;
            if (slot) det = track_slot_update(st, t, my, free_set, unmatched, issued, s_det, 3, p, &fresh, &Te);
            s_fresh[t] = fresh ? 1 : 0;
            s_te[t] = Te;
            s_ad[t] = det >= 0 && !fresh ? track_alpha(p.d_cutoff, Te) : 0.0;
            s_slot_id[t] = slot ? st.id[t] : 0;
            if (det >= 0) s_det_slot[det] = t;  // det < P; distinct slots hold distinct rows
            if (tid == 0) {
                const int nfree = track_popcount(free_set), nun = track_popcount(unmatched);
                st.hdr[0] = issued + (nun < nfree ? nun : nfree);
                st.hdr[1] += 1;
                out_flags[b] = (fl & HH_DECODE_SOLVER_GUARD ? HH_TRACK_SOLVER_GUARD : 0) | (nun > nfree ? HH_TRACK_POOL_FULL : 0);
            }
        }
        __syncthreads();
        for (int e = tid; e < P * K; e += TRACK_THREADS) {
            const int d = e / K, k = e % K, t = s_det_slot[d];
            const float *det = s_det + (size_t)d * K * 3;
            float o[2];
            if (t >= 0) track_joint_update(st, t, k, det, 3, s_fresh[t] != 0, s_te[t], s_ad[t], p, o);
            else { o[0] = det[k * 3]; o[1] = det[k * 3 + 1]; }
            smooth[(b * P * K + e) * 2] = o[0];
            smooth[(b * P * K + e) * 2 + 1] = o[1];
        }
        if (tid < P) track_ids[b * P + tid] = s_det_slot[tid] >= 0 ? s_slot_id[s_det_slot[tid]] : 0;
        __syncthreads();
    }
    if (lds_state)
        for (int i = tid; i < words; i += TRACK_THREADS) reinterpret_cast<uint64_t *>(home)[i] = reinterpret_cast<const uint64_t *>(base)[i];
}

// hh_track_assign: one wave per matrix, straight from global memory.
__global__ __launch_bounds__(64) void track_assign_kernel(const double *__restrict__ sim, const int32_t *__restrict__ ids, int T, int P, double min_oks,
                                                          int32_t *__restrict__ match)
{
    const int t = threadIdx.x;
    const size_t m = blockIdx.x;  // m < n = the grid's size
    uint64_t taken;
    const int my = track_wave_assign(sim + m * T * P, t, P, t < T ? ids[m * T + t] : 0, min_oks, &taken);
    if (t < T) match[m * T + t] = my;
}

static hipError_t track_launch(int mode, const TrackParams &p, void *state, const float *joints, const float *scores, const int32_t *num_people,
                               const int32_t *flags, int S, int F, int32_t *track_ids, float *smooth, int32_t *out_flags, double *sim_out, hipStream_t s)
{
    if (S == 0 || F == 0) return hipSuccess;
    static bool attr_set[64] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (!attr_set[dev & 63]) {
        if ((e = hipFuncSetAttribute(reinterpret_cast<const void *>(track_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, TRACK_LDS_BUDGET)) != hipSuccess) return e;
        attr_set[dev & 63] = true;
    }
    const int64_t bytes = track_state_bytes(p.K, p.max_tracks);
    const int64_t sim_bytes = ((int64_t)p.max_tracks * p.max_people * 8 + (int64_t)p.max_people * p.K * 12 + 7) & ~(int64_t)7;  // similarities, staged rows
    const int lds_state = !(p.reserved & 1) && sim_bytes + bytes <= TRACK_LDS_BUDGET;
    const size_t lds = (size_t)(sim_bytes + (lds_state ? bytes : 0));
    hipLaunchKernelGGL(track_kernel, dim3(S), dim3(TRACK_THREADS), lds, s, p, (unsigned char *)state, (long long)bytes, joints, scores, num_people, flags, F, mode,
                       lds_state, track_ids, smooth, out_flags, sim_out);
    return hipGetLastError();
}

hipError_t launch_track_step(const TrackParams &p, void *state, const float *joints, const float *scores, const int32_t *num_people, const int32_t *flags, int S,
                             int F, int32_t *track_ids, float *smooth, int32_t *out_flags, hipStream_t s)
{
    return track_launch(TRACK_MODE_STEP, p, state, joints, scores, num_people, flags, S, F, track_ids, smooth, out_flags, nullptr, s);
}

hipError_t launch_track_similarity(const TrackParams &p, void *state, const float *joints, const float *scores, const int32_t *num_people, const int32_t *flags,
                                   int S, double *sim, hipStream_t s)
{
    return track_launch(TRACK_MODE_SIM, p, state, joints, scores, num_people, flags, S, 1, nullptr, nullptr, nullptr, sim, s);
}

hipError_t launch_track_assign(const double *sim, const int32_t *ids, int n, int T, int P, double min_oks, int32_t *match, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(track_assign_kernel, dim3(n), dim3(64), 0, s, sim, ids, T, P, min_oks, match);
    return hipGetLastError();
}

void track_step_host(const TrackParams &p, void *state, const float *joints, const float *scores, const int32_t *num_people, const int32_t *flags, int S, int F,
                     int32_t *track_ids, float *smooth, int32_t *out_flags)
{
    const int64_t bytes = track_state_bytes(p.K, p.max_tracks);
    const size_t P = p.max_people, K = p.K, W = 3 + p.E;
    double *sim = new double[(size_t)p.max_tracks * P];
    for (int s = 0; s < S; ++s)
        for (int f = 0; f < F; ++f) {
            const size_t b = (size_t)s * F + f;
            track_frame_host(p, (unsigned char *)state + (size_t)s * bytes, joints + b * P * K * W, scores + b * P, num_people[b], flags ? flags[b] : 0,
                             track_ids + b * P, smooth + b * P * K * 2, out_flags + b, sim);
        }
    delete[] sim;
}
