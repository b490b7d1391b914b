// The tracker's code (pytorch-human-pose_amd/csrc/track_math.h: validity, similarity, greedy assignment, slot bookkeeping, One-Euro update,
// one frame in plain loops) compiled for the HOST and run over generated clips, so that the address arithmetic can be put under the
// sanitizers without a GPU:
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I pytorch-human-pose_amd/csrc tools/track_host_check.cpp -o /tmp/track_host_check && /tmp/track_host_check
//
// Every buffer is its own heap block of exactly its size (state, joints, scores, counts, flags, ids, smooth, out_flags, the similarity
// scratch), so a read or write one element past any of them is an AddressSanitizer report.  The shapes are the limits and the odd ones:
// K in {1, 5, 17, 64}, max_tracks in {1, 4, 33, 64}, max_people in {1, 30, 64}, num_people from 0 to max_people (and beyond it, and
// negative: clamped), E in {0, 1, 3}.  Checked besides: ids are 0 or positive and unique within a frame, never larger than the number
// issued, an id seen on a row was never seen before unless it was live; every smooth element was written (a NaN canary is gone); chunked
// (frame by frame) and whole-clip walks leave the same state; the assignment on tie-ridden matrices never matches a detection twice.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "track_math.h"

static unsigned long long rng_state = 88172645463325252ull;
static double urand()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (double)(rng_state >> 11) / 9007199254740992.0;
}

template <class T> struct Buf {  // exactly n elements, nothing behind them
    T *ptr;
    size_t n;
    explicit Buf(size_t n_) : ptr((T *)malloc(n_ ? n_ * sizeof(T) : 1)), n(n_) { if (!ptr) abort(); }
    ~Buf() { free(ptr); }
};

static int run(int K, int T, int P, int E, int frames, int people)
{
    TrackParams p;
    memset(&p, 0, sizeof p);
    for (int k = 0; k < K; ++k) p.vars[k] = 0.01 + 0.002 * (k % 5);
    p.fps = 30.0, p.min_cutoff = 1.0, p.beta = 0.007, p.d_cutoff = 1.0, p.min_oks = 0.3;
    p.joint_thr = 0.05f, p.min_person_score = 0.0f;
    p.K = K, p.E = E, p.max_people = P, p.max_tracks = T, p.max_age = 2, p.min_joints = K < 3 ? 1 : 3, p.min_common = K < 3 ? 1 : 3;
    if (track_check(&p)) { printf("parameters refused: %s\n", track_check(&p)); return 1; }
    const size_t W = 3 + E, row = (size_t)K * W, bytes = (size_t)track_state_bytes(K, T);
    Buf<unsigned char> state(bytes), state2(bytes);
    memset(state.ptr, 0, bytes);
    memset(state2.ptr, 0, bytes);
    Buf<float> joints((size_t)frames * P * row), scores((size_t)frames * P), smooth((size_t)frames * P * K * 2), smooth2((size_t)frames * P * K * 2);
    Buf<int32_t> num(frames), flags(frames), ids((size_t)frames * P), ids2((size_t)frames * P), out_flags(frames), out_flags2(frames);
    Buf<double> sim((size_t)T * P);
    // `people` persons drift on a grid; each frame lists them in a rotated order; some frames are empty, over-full, fallback or guard
    std::vector<double> cx(people), cy(people);
    for (int q = 0; q < people; ++q) cx[q] = 60.0 + 90.0 * (q % 8) + 5 * urand(), cy[q] = 60.0 + 90.0 * (q / 8) + 5 * urand();
    for (int f = 0; f < frames; ++f) {
        int n = people < P ? people : P;
        if (f % 7 == 5) n = 0;
        for (int d = 0; d < P; ++d) {
            const int q = n ? (d + f) % n : 0;
            float *j = joints.ptr + ((size_t)f * P + d) * row;
            for (int k = 0; k < K; ++k) {
                j[k * W] = (float)(cx[q] + 20.0 * std::sin(0.7 * k) + 0.4 * f + 0.2 * urand());
                j[k * W + 1] = (float)(cy[q] + 25.0 * std::cos(1.3 * k) + 0.2 * urand());
                j[k * W + 2] = d < n ? ((f + k + q) % 11 == 0 ? 0.01f : 0.6f) : 0.f;
                for (int e = 0; e < E; ++e) j[k * W + 3 + e] = (float)q;
            }
            scores.ptr[(size_t)f * P + d] = d < n ? 0.5f : 0.f;
        }
        num.ptr[f] = f % 9 == 4 ? P + 3 : (f % 9 == 8 ? -2 : n);  // beyond the table and negative: clamped
        flags.ptr[f] = f % 10 == 6 ? HH_DECODE_FALLBACK : (f % 10 == 9 ? HH_DECODE_SOLVER_GUARD : 0);
    }
    for (size_t i = 0; i < smooth.n; ++i) smooth.ptr[i] = smooth2.ptr[i] = NAN;
    int bad = 0;
    // frame by frame
    std::vector<char> seen(1 << 20, 0), live_prev(1 << 20, 0);
    for (int f = 0; f < frames; ++f) {
        track_frame_host(p, state.ptr, joints.ptr + (size_t)f * P * row, scores.ptr + (size_t)f * P, num.ptr[f], flags.ptr[f], ids.ptr + (size_t)f * P,
                         smooth.ptr + (size_t)f * P * K * 2, out_flags.ptr + f, sim.ptr);
        const int issued = ((const int32_t *)state.ptr)[0];
        std::vector<char> live_now(1 << 20, 0);
        for (int d = 0; d < P; ++d) {
            const int id = ids.ptr[(size_t)f * P + d];
            if (id == 0) continue;
            if (id < 0 || id > issued || live_now[id]) { ++bad; continue; }
            if (seen[id] && !live_prev[id]) ++bad;  // an expired id came back
            live_now[id] = 1;
            seen[id] = 1;
        }
        const TrackState st = track_state_view(state.ptr, K, T);
        std::fill(live_prev.begin(), live_prev.end(), 0);
        for (int t = 0; t < T; ++t) {
            if (st.id[t] < 0 || st.id[t] > issued) ++bad;
            if (st.id[t]) { if (live_prev[st.id[t]]) ++bad; live_prev[st.id[t]] = 1; }  // one slot per id
            if (st.id[t] && st.misses[t] > p.max_age) ++bad;
        }
        if ((flags.ptr[f] & HH_DECODE_SOLVER_GUARD) && !(out_flags.ptr[f] & HH_TRACK_SOLVER_GUARD)) ++bad;
    }
    for (size_t i = 0; i < smooth.n; ++i) bad += std::isnan(smooth.ptr[i]) ? 1 : 0;
    // the whole clip in one walk: the same bytes
    for (int f = 0; f < frames; ++f)
        track_frame_host(p, state2.ptr, joints.ptr + (size_t)f * P * row, scores.ptr + (size_t)f * P, num.ptr[f], flags.ptr[f], ids2.ptr + (size_t)f * P,
                         smooth2.ptr + (size_t)f * P * K * 2, out_flags2.ptr + f, sim.ptr);
    bad += memcmp(state.ptr, state2.ptr, bytes) != 0;
    bad += memcmp(ids.ptr, ids2.ptr, ids.n * 4) != 0;
    bad += memcmp(smooth.ptr, smooth2.ptr, smooth.n * 4) != 0;
    // the assignment on matrices full of ties
    Buf<int32_t> tid(T), match(T);
    for (int round = 0; round < 8; ++round) {
        for (int t = 0; t < T; ++t) tid.ptr[t] = urand() < 0.2 ? 0 : t * 3 + 1;
        for (size_t i = 0; i < sim.n; ++i) sim.ptr[i] = round == 0 ? 0.5 : std::floor(urand() * 4) / 4.0;
        uint64_t taken = 0, check = 0;
        track_assign_host(sim.ptr, tid.ptr, T, P, 0.25, match.ptr, &taken);
        for (int t = 0; t < T; ++t) {
            const int d = match.ptr[t];
            if (d < -1 || d >= P) { ++bad; continue; }
            if (d < 0) continue;
            if (tid.ptr[t] == 0 || ((check >> d) & 1) || sim.ptr[(size_t)t * P + d] < 0.25) ++bad;
            check |= (uint64_t)1 << d;
        }
        bad += check != taken;
    }
    printf("K %2d  T %2d  P %2d  E %d  frames %d  people %2d: issued %d, %d problems\n", K, T, P, E, frames, people, ((const int32_t *)state.ptr)[0], bad);
    return bad;
}

int main()
{
    int bad = 0;
    const int Ks[] = {1, 5, 17, 64}, Ts[] = {1, 4, 33, 64}, Ps[] = {1, 30, 64}, Es[] = {0, 1, 3};
    int i = 0;
    for (int K : Ks)
        for (int T : Ts)
            for (int P : Ps) bad += run(K, T, P, Es[i++ % 3], 23, P < 40 ? P : 40);
    bad += run(17, 64, 30, 1, 40, 6);
    bad += run(64, 64, 64, 1, 12, 64);
    printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
