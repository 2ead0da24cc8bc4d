// dvo_map_kernels.hip -- the mapping half of the hot path (src/map/mapper.cpp, src/map/implement.cpp) as gfx950 kernels, for
// n_seq sequences per launch.  Maps are [n_seq][h][w] blocks of the top pyramid level; the workgroup index carries the sequence
// (grid.x = workgroups per sequence * n_seq) and every kernel that belongs to one branch of Mapper::estimate (mapper.cpp:16-33)
// starts by reading its sequence's need flag -- one scalar load -- and leaves if the sequence took the other branch.
// The same kernels serve the single-sequence dvo_vo handle (n_seq = 1) and the operator-level entry points.
// Built with -ffp-contract=off: only the fmaf() calls written here and in dvo_math.h fuse.
#include <hip/hip_runtime.h>

#include "dvo_kernels.h"

namespace dvo {

static inline unsigned cdiv_u(unsigned a, unsigned b) { return (a + b - 1) / b; }

// (sequence, pixel) of a thread; false when the thread has no pixel.  Grid = seq_grid() (dvo_kernels.h): the sequence is
// (blockIdx.z, blockIdx.y), no division.
__device__ __forceinline__ int grid_seq() { return (int)(blockIdx.z * DVO_GRID_SEQ_Y + blockIdx.y); }
__device__ __forceinline__ bool seq_pixel(int npix, int n_seq, int& seq, int& i)
{
    seq = grid_seq();
    i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    return (i < npix) & (seq < n_seq);
}
// y = i / w, x = i % w for 0 <= i < 2^24 through the reciprocal (the +-1 fix-up is branch free)
__device__ __forceinline__ void split_row(int i, int w, float inv_w, int& x, int& y)
{
    y = (int)((float)i * inv_w);
    x = i - y * w;
    const int lo = x < 0 ? 1 : 0, hi = x >= w ? 1 : 0;
    y += hi - lo;
    x += (lo - hi) * w;
}

// Per-camera mono batches (dvo_batch_create_mono_cameras): the intrinsics a mapping kernel uses for its sequence -- a.k, or (PCAM:
// the per-camera kernels) `cam`, the sequence's entry of the per-sequence table, loaded once per workgroup.  Called at each use,
// with a.k not bound to a local, as seq_intr in dvo_kernels.hip: PCAM = false is then the code the kernel always was.
template <bool PCAM, class Args>
__device__ __forceinline__ const Intr& map_intr(const Args& a, const Intr& cam)
{
    if constexpr (PCAM) return cam;
    else return a.k;
}

// ------------------------------------------------------------------------------------------------
// k_mono_decide: what System::VisualOdometry::odometrize does between Tracker::track and Mapper::estimate
// (system.hpp:57-73, frame.cpp:7-14, mapper.cpp:45-60), one thread per sequence, in the double-precision pose algebra of
// dvo_math.h: rel_xi <- the tracker's twist, frame_xi <- concatenate(ref_xi, rel_xi), need <- needNewFrame,
// rel_pose <- exp(+rel_xi), T_world <- exp(frame_xi).
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_mono_decide(MonoSeq* meta, const SeqState* state, int n_seq, int frame_id, float min_translation,
                                                    int max_frames, float* xi_world, float* T_world, int* is_key, MonoRef host_ref, int* need_list)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n_seq) return;
    MonoSeq& m = meta[s];
    if (host_ref.valid) {   // a dvo_vo handle keeps FrameHistory on the host: the reference keyframe's pose / id arrive as kernel arguments
        for (int i = 0; i < 6; i++) m.ref_xi[i] = host_ref.ref_xi[i];
        m.ref_id = host_ref.ref_id; m.n_total = host_ref.n_total;
    }
    const int need = mono_track_one(m, state[s], frame_id, min_translation, max_frames, s, xi_world, T_world, is_key);
    if (need && need_list) need_list[4 + atomicAdd(&need_list[0], 1)] = s;   // (the order of the list changes no result: sequences are independent)
}

// k_mono_commit: FrameHistory::setRefFrame / push (frame.hpp:151-157) for the sequences that created a keyframe: the frame's
// pose becomes the reference pose and enters the ring.  all = 1: first frame (identity pose, every sequence; the frame id is the
// caller's and MonoSeq::clamped is left as it is).
__global__ void __launch_bounds__(64) k_mono_commit(MonoSeq* meta, float* hist_xi, int n_seq, int R, int all, int frame_id, float* xi_world,
                                                    float* T_world, int* is_key)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n_seq) return;
    MonoSeq& m = meta[s];
    float* ring = hist_xi + (size_t)s * R * 6;
    if (all) mono_start_one(m, frame_id, ring, s, xi_world, T_world, is_key);
    else if (m.need) mono_frame_to_ref(m, ring, R);
}

// k_mono_decide_plan / k_mono_commit_plan: k_mono_decide and k_mono_commit of a planned mono call (dvo_batch_set_mono_actions).
// A TRACK sequence does exactly what they do, with its own next frame id (frame ids count from each start).  A sequence that does
// not track parks its need flag in need_save and raises it, so that k_age_table and k_depth_update leave it alone (and it is never in
// need_list: k_propagate_* and k_promote do not see it); k_mono_commit_plan puts the flag back.  SKIP keeps its world pose (identity
// while it has never started) with is_keyframe = 0; RESTART becomes frame 0 of its sequence, its counters reset.
__global__ void __launch_bounds__(64) k_mono_decide_plan(MonoPlanArgs a)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= a.n_seq) return;
    MonoSeq& m = a.meta[s];
    if (a.eff[s] == DVO_SEQ_TRACK) {
        const int need = mono_track_one(m, a.state[s], m.frame_id + 1, a.min_translation, a.max_frames, s, a.xi_world, a.T_world, a.is_key);
        if (need) a.need_list[4 + atomicAdd(&a.need_list[0], 1)] = s;
        return;
    }
    a.need_save[s] = m.need;
    m.need = 1;
    a.is_key[s] = 0;
    if (!a.started[s]) mono_identity_world(s, a.xi_world, a.T_world);
}

__global__ void __launch_bounds__(64) k_mono_commit_plan(MonoPlanArgs a)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= a.n_seq) return;
    MonoSeq& m = a.meta[s];
    const int eff = a.eff[s];
    float* ring = a.hist_xi + (size_t)s * a.R * 6;
    if (eff == DVO_SEQ_RESTART) {
        mono_start_one(m, 0, ring, s, a.xi_world, a.T_world, a.is_key);
        m.clamped = 0;
        a.started[s] = 1;
    } else if (eff != DVO_SEQ_TRACK) {
        m.need = a.need_save[s];
    } else if (m.need) {
        mono_frame_to_ref(m, ring, a.R);
    }
}

// k_kf_decide: the keyframe bookkeeping of a sensor-depth batch with keyframe tracking (dvo_batch_set_keyframe_tracking, DESIGN.md
// §19), after the push's tracking.  TRACK tracks with the sequence's next frame id and, when the rule fires, makes the frame the
// reference at once; RESTART starts the sequence as frame 0, its counters reset.  Both enter need_list, whose frames k_promote then
// copies over the keyframe set.  SKIP changes nothing: its world pose stays (identity while the sequence has never started,
// n_total = 0), is_keyframe = 0.  There is no ring and nothing between this kernel and the copy reads MonoSeq, so decide and commit
// are one launch (no need_save, no started array).
__global__ void __launch_bounds__(64) k_kf_decide(MonoPlanArgs a)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= a.n_seq) return;
    MonoSeq& m = a.meta[s];
    const int eff = a.eff[s];
    if (eff == DVO_SEQ_TRACK) {
        if (!mono_track_one(m, a.state[s], m.frame_id + 1, a.min_translation, a.max_frames, s, a.xi_world, a.T_world, a.is_key)) return;
        mono_frame_to_ref(m, nullptr, 1);
    } else if (eff == DVO_SEQ_RESTART) {
        mono_start_one(m, 0, nullptr, s, a.xi_world, a.T_world, a.is_key);
        m.clamped = 0;
    } else {
        a.is_key[s] = 0;
        if (m.n_total == 0) mono_identity_world(s, a.xi_world, a.T_world);
        return;
    }
    a.need_list[4 + atomicAdd(&a.need_list[0], 1)] = s;   // (the order of the list changes no result: sequences are independent)
}

// k_mono_seed: the start pose of a mono call (dvo_batch_set_pose_guess_mode), after k_track_begin / k_plan.  History: the world
// twists w1 (newest), w2 returned for the sequence's last two calls that tracked or started it since its last start.  A guess g in
// world coordinates becomes the tracker's relative start concatenate(-ref_xi, g) against the sequence's current keyframe.
__global__ void __launch_bounds__(64) k_mono_seed(PoseSeedArgs a)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= a.n_seq) return;
    float* w = a.hist + (size_t)s * 12;   // w1 = w[0..5], w2 = w[6..11]
    int n = a.hist_n[s];
    const int pe = a.prev_eff[s];
    if (pe == DVO_SEQ_TRACK) {
        for (int i = 0; i < 6; i++) { w[6 + i] = w[i]; w[i] = a.last_xi[(size_t)s * 6 + i]; }
        n = n < 2 ? n + 1 : 2;
    } else if (pe == DVO_SEQ_RESTART) {
        for (int i = 0; i < 6; i++) w[i] = a.last_xi[(size_t)s * 6 + i];
        n = 1;
    }
    a.hist_n[s] = (uint8_t)n;
    const int eff = a.eff ? (int)a.eff[s] : a.all_eff;
    a.prev_eff[s] = (uint8_t)eff;
    float x[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (eff == DVO_SEQ_TRACK) {
        float g[6];
        bool have = false;
        if (a.mode == DVO_GUESS_GIVEN && a.rows) {
            have = true;
            for (int i = 0; i < 6; i++) { g[i] = a.rows[(size_t)s * 6 + i]; have = have && isfinite(g[i]); }
        } else if (a.mode == DVO_GUESS_CONSTANT_VELOCITY && n >= 2) {
            float w1[6], nw2[6], d[6];
            for (int i = 0; i < 6; i++) { w1[i] = w[i]; nw2[i] = -w[6 + i]; }
            se3_concatenate_f(nw2, w1, d);
            se3_concatenate_f(w1, d, g);
            have = true;
        }
        if (have) {
            float nref[6];
            for (int i = 0; i < 6; i++) nref[i] = -a.meta[s].ref_xi[i];
            se3_concatenate_f(nref, g, x);
        }
    }
    seed_state(a.state[s], x, a.start + (size_t)s * 6);
}

// k_age_table: the per-keyframe part of Mapper::update (mapper.cpp:99-107) hoisted out of the pixel loop: for every retained
// keyframe, r_xi = concatenate(obj.xi, -born.xi), the pose exp(-r_xi) that the epipolar search warps with and -r_xi's
// translation (implement.cpp:56).  One thread per (sequence, history index).
__global__ void __launch_bounds__(64) k_age_table(AgeTableArgs a)
{
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t == 0 && a.zero_word) *a.zero_word = 0;
    if (t >= a.n_seq * a.R) return;
    const int seq = t / a.R, i = t - seq * a.R;
    const MonoSeq& m = a.meta[seq];
    int n_hist, slot;
    if (a.n_hist >= 0) {          // single handle: the table is the whole FrameHistory, slot = history index
        n_hist = a.n_hist; slot = i;
    } else {                      // ring: the newest min(n_total, R) keyframes
        if (m.need) return;       // (sequences that create a keyframe do not search)
        n_hist = m.n_total < a.R ? m.n_total : a.R;
        slot = (m.n_total - n_hist + i) % a.R;
    }
    if (i >= n_hist) return;
    AgeEntry e;
    age_entry_one(m.frame_xi, a.hist_xi + ((size_t)seq * a.R + slot) * 6, slot, e);
    a.ages[(size_t)seq * a.R + i] = e;
}

// ------------------------------------------------------------------------------------------------
// Implement::propagate (implement.cpp:217-256).  The reference's forEach scatter races; its sequential semantics are "last
// writer in raster order wins" (D7).  Three passes reproduce that exactly:
//   pass 0: outputs <- (1, 1, 0), owner <- -1;  pass 1: owner[target] = max(source index);
//   pass 2: every target pulls depth/sigma/age from its owning source pixel.
// ------------------------------------------------------------------------------------------------
// (four pixels per thread: on most frames most sequences take the other branch, and a workgroup that only finds that out costs
//  as much to dispatch as one that works -- a quarter of the workgroups)
#define DVO_PROP_PER_THREAD 4
#define DVO_LIST_SLOTS 1024   /* sequence slots of a launch that works through a compact list (PropArgs::need_list) */
__device__ __forceinline__ int prop_chunk(int& seq)   // first pixel of this thread (stride 256), sequence of the workgroup
{
    seq = grid_seq();
    return (int)blockIdx.x * (256 * DVO_PROP_PER_THREAD) + (int)threadIdx.x;
}

// The sequences a workgroup of the propagate / promote kernels works through: with a list, slot j takes entries j, j + n_slots, ...;
// without one, its own sequence (when the `need` flag says so).  Returns false when there is nothing (more) to do.
__device__ __forceinline__ bool next_listed_seq(const int* list, int n_slots, int n_seq, const MonoSeq* meta, int& cursor, int& seq)
{
    if (list) {
        if (cursor < 0) cursor = grid_seq(); else cursor += n_slots;
        if (cursor >= list[0]) return false;
        seq = list[4 + cursor];
        return true;
    }
    if (cursor >= 0) return false;
    cursor = 0;
    seq = grid_seq();
    return seq < n_seq && !(meta && !meta[seq].need);
}

__global__ void __launch_bounds__(256) k_propagate_init(PropArgs a)
{
    int seq, cursor = -1;
    const int n = a.w * a.h, i0 = prop_chunk(seq);
    while (next_listed_seq(a.need_list, a.n_slots, a.n_seq, a.meta, cursor, seq)) {
#pragma unroll
        for (int k = 0; k < DVO_PROP_PER_THREAD; k++) {
            const int i = i0 + k * 256;
            if (i >= n) break;
            const size_t o = (size_t)seq * n + i;
            a.depth[o] = 1.0f; a.sigma[o] = 1.0f; a.age[o] = 0.0f; a.owner[o] = -1;
        }
    }
}

// PCAM: per-sequence intrinsics (PropArgs::seq_k, k_propagate_owner_cam).  The arguments are taken by value: by reference, the
// default kernel's instruction stream changed.
template <bool PCAM>
__device__ __forceinline__ void propagate_owner(PropArgs a)
{
    int seq, cursor = -1;
    const int w = a.w, h = a.h, n = w * h, i0 = prop_chunk(seq);
    while (next_listed_seq(a.need_list, a.n_slots, a.n_seq, a.meta, cursor, seq)) {
        const Pose pose = a.meta ? a.meta[seq].rel_pose : a.pose;   // wave-uniform
        Intr cam;
        if constexpr (PCAM) cam = load_seq_entry(a.seq_k, seq);
#pragma unroll
        for (int k = 0; k < DVO_PROP_PER_THREAD; k++) {
            const int i = i0 + k * 256;
            if (i >= n) break;
            int x, y;
            split_row(i, w, a.inv_w, x, y);
            const float rd = a.ref_depth[(size_t)seq * n + i];
            if (is_epsilon(rd)) continue;
            float pu, pv;
            warp(pose, map_intr<PCAM>(a, cam), (float)x, (float)y, rd, pu, pv);
            int qx, qy;
            if (!round_coord(pu, qx) || !round_coord(pv, qy)) continue;
            if (qx < 0 || w <= qx || qy < 0 || h <= qy) continue;
            atomicMax(&a.owner[(size_t)seq * n + qy * w + qx], i);
        }
    }
}

__global__ void __launch_bounds__(256) k_propagate_owner(PropArgs a) { propagate_owner<false>(a); }
__global__ void __launch_bounds__(256) k_propagate_owner_cam(PropArgs a) { propagate_owner<true>(a); }

__global__ void __launch_bounds__(256) k_propagate_pull(PropArgs a)
{
    int seq, cursor = -1;
    const int n = a.w * a.h, o0 = prop_chunk(seq);
    while (next_listed_seq(a.need_list, a.n_slots, a.n_seq, a.meta, cursor, seq)) {
        const float tz = a.meta ? a.meta[seq].rel_xi[2] : a.tz;
        const size_t base = (size_t)seq * n;
#pragma unroll
        for (int k = 0; k < DVO_PROP_PER_THREAD; k++) {
            const int o = o0 + k * 256;
            if (o >= n) break;
            const int i = a.owner[base + o];
            if (i < 0) continue;
            const float rd = a.ref_depth[base + i];
            float s = a.ref_sigma[base + i];
            const float d0 = rd < 0.01f ? 0.01f : rd;
            const float d1 = d0 + tz;
            const float q = d1 / d0;
            const float q4 = q * (q * (q * q));          // math::pow(q, 4), util.hpp:19-27
            s = sqrtf(fmaf(q4, s * s, 0.06f * 0.06f));   // implement.cpp:246-247
            a.depth[base + o] = d1 < 0.0f ? 0.0f : d1;
            a.sigma[base + o] = s;
            a.age[base + o] = a.ref_age[base + i] + 1.0f;
        }
    }
}

// The four neighbour fusions of Implement::regularize (implement.cpp:166-177), order L, R, D, U.  All eight neighbour loads are
// issued before the first fusion (from the centre's address where a neighbour does not exist; that value is not used): the fusions
// are a dependent chain, and with each load inside its own `if` the kernel paid four exposed memory round trips per pixel.
__device__ __forceinline__ void regularize_fuse4(const float* __restrict__ depth, const float* __restrict__ sigma, int i, int x, int y, int w, int h,
                                                 float& gd, float& gs)
{
    const bool hasL = x - 1 >= 0, hasR = x + 1 < w, hasD = y + 1 < h, hasU = y - 1 >= 0;
    const int iL = hasL ? i - 1 : i, iR = hasR ? i + 1 : i, iD = hasD ? i + w : i, iU = hasU ? i - w : i;
    const float dL = depth[iL], sL = sigma[iL], dR = depth[iR], sR = sigma[iR];
    const float dD = depth[iD], sD = sigma[iD], dU = depth[iU], sU = sigma[iU];
    // Are all ten operands positive normal floats in [2^-20, 2^20]?  As unsigned integers their bit patterns order like the floats,
    // negative values, infinities and NaNs lie above every positive finite one, zeros and subnormals below 2^-20: one min / max tree.
    // (A neighbour that does not exist was loaded from the centre: in range if the centre is.)  Then the eight divisions and four
    // square roots of the fusions take their verified short forms (dvo_math.h); otherwise -- a wave-uniform branch no real map takes --
    // the IEEE sequences.  Same bits either way.
#if defined(__HIP_DEVICE_COMPILE__)
    const unsigned b0 = __float_as_uint(gd), b1 = __float_as_uint(gs), b2 = __float_as_uint(dL), b3 = __float_as_uint(sL), b4 = __float_as_uint(dR),
                   b5 = __float_as_uint(sR), b6 = __float_as_uint(dD), b7 = __float_as_uint(sD), b8 = __float_as_uint(dU), b9 = __float_as_uint(sU);
    const unsigned lo = min(min(min(b0, b1), min(b2, b3)), min(min(b4, b5), min(min(b6, b7), min(b8, b9))));
    const unsigned hi = max(max(max(b0, b1), max(b2, b3)), max(max(b4, b5), max(max(b6, b7), max(b8, b9))));
    const bool ranged = (lo >= DVO_FUSE_RANGE_LO) & (hi <= DVO_FUSE_RANGE_HI);
    if (__builtin_amdgcn_ballot_w64(!ranged) == 0ull) {
        if (hasL) gaussian_fuse_ranged(gd, gs, dL, sL);
        if (hasR) gaussian_fuse_ranged(gd, gs, dR, sR);
        if (hasD) gaussian_fuse_ranged(gd, gs, dD, sD);
        if (hasU) gaussian_fuse_ranged(gd, gs, dU, sU);
        return;
    }
    asm volatile("; regularize_fuse4: IEEE division / square root");
#endif
    if (hasL) gaussian_fuse(gd, gs, dL, sL);
    if (hasR) gaussian_fuse(gd, gs, dR, sR);
    if (hasD) gaussian_fuse(gd, gs, dD, sD);
    if (hasU) gaussian_fuse(gd, gs, dU, sU);
}

// Implement::regularize (implement.cpp:156-180): reads the old maps, fuses L, R, D, U in that order.
__global__ void __launch_bounds__(256) k_regularize(const float* __restrict__ depth_all, const float* __restrict__ sigma_all, int w, int h,
                                                    int n_seq, float inv_w, float* __restrict__ out_all)
{
    int seq, i;
    if (!seq_pixel(w * h, n_seq, seq, i)) return;
    const size_t base = (size_t)seq * w * h;
    const float* __restrict__ depth = depth_all + base;
    const float* __restrict__ sigma = sigma_all + base;
    int x, y;
    split_row(i, w, inv_w, x, y);
    float gd = depth[i], gs = sigma[i];
    regularize_fuse4(depth, sigma, i, x, y, w, h, gd, gs);
    out_all[base + i] = gd < 6.0f ? gd : 6.0f;
}

// k_regularize_redecimate: k_regularize and the re-decimation that follows it in the mono pipeline, one pass.  Same operations per
// pixel as k_regularize + k_pyramid(culls = 0, depth and sigma): the regularized value is written to a second top-level buffer (the
// 5-point stencil of the neighbours still reads the old one) and decimated on the spot into every level it lands on, with sigma,
// and the Gauss-Newton weight -- saves one launch and the 8 B/px round trip of the intermediate map.
// (the arguments by value, as in propagate_owner: k_regularize_redecimate is the code it always was)
__device__ __forceinline__ void regularize_redecimate_px(RegDecArgs a, int seq, int i)
{
    const int T = a.levels - 1, w = a.w[T], h = a.h[T];
    const size_t base = (size_t)seq * w * h;
    const float* __restrict__ depth = a.depth + base;
    const float* __restrict__ sigma = a.sigma + base;
    int x, y;
    split_row(i, w, a.inv_w, x, y);
    const float s0 = sigma[i];
    float gd = depth[i], gs = s0;
    regularize_fuse4(depth, sigma, i, x, y, w, h, gd, gs);
    const float nd = gd < 6.0f ? gd : 6.0f;                       // implement.cpp:178
    a.depth_top_out[base + i] = nd;                               // top level: the map itself (cullImage(src, 0) aliases, convert.cpp:9-10)
    __builtin_nontemporal_store(gn_weight(a.step[T], a.sigma_min, a.sigma_max, s0), a.wgt[T] + base + i);
    const float vd = pass_valid(nd), vs = pass_valid(s0);
    for (int t = 1; t < a.levels; t++) {                          // lower levels keep pixels whose coordinates are multiples of 2^t
        const int msk = (1 << t) - 1;
        if ((x & msk) | (y & msk)) break;
        const int l = T - t, lx = x >> t, ly = y >> t;
        if (lx >= a.w[l] || ly >= a.h[l]) continue;
        const size_t o = (size_t)seq * a.w[l] * a.h[l] + (size_t)ly * a.w[l] + lx;
        a.depth_lv[l][o] = vd;
        a.sigma_lv[l][o] = vs;
        a.wgt[l][o] = gn_weight(a.step[l], a.sigma_min, a.sigma_max, vs);
    }
}

__global__ void __launch_bounds__(256) k_regularize_redecimate(RegDecArgs a)
{
    const int T = a.levels - 1;
    int seq, i;
    if (!seq_pixel(a.w[T] * a.h[T], a.n_seq, seq, i)) return;
    regularize_redecimate_px(a, seq, i);
}

// k_regularize_redecimate_plan: a planned mono call (dvo_batch_set_mono_actions).  The action is uniform per workgroup (seq_grid).
//  TRACK    k_regularize_redecimate's pixel.
//  SKIP     the top-level depth is copied forward into depth_top_out (the host swaps the two buffers after this launch); nothing
//           else of the keyframe is touched: it is not regularised.
//  RESTART  what the first frame does (system.hpp:49-54, MonoBatch::odometrize's frame-0 branch): the frame's gray pyramid becomes
//           the keyframe's and enters ring slot 0, age 0, and the start map is re-decimated with the operations of redecimate()
//           (k_pyramid with culls = 0: the top level as given, pass_valid below, the weight of the level's sigma).
//           Start map: the per-call rows when set; else, on a sequence's first start, its own top-level maps (what
//           dvo_batch_set_initial_depth / _device or the default left there, kept by the copy-forward); else init_depth / init_sigma.
__global__ void __launch_bounds__(256) k_regularize_redecimate_plan(RegDecArgs a, MonoStartArgs p)
{
    const int T = a.levels - 1, w = a.w[T], h = a.h[T];
    int seq, i;
    if (!seq_pixel(w * h, a.n_seq, seq, i)) return;
    // the action byte through a scalar load of its aligned word (the sequence is uniform per workgroup; eff is padded to 4 bytes)
    const int eff = (int)((load_seq_entry(reinterpret_cast<const uint32_t*>(p.eff), seq >> 2) >> ((seq & 3) * 8)) & 0xffu);
    if (eff == DVO_SEQ_TRACK) { regularize_redecimate_px(a, seq, i); return; }
    const size_t base = (size_t)seq * w * h;
    if (eff != DVO_SEQ_RESTART) { a.depth_top_out[base + i] = a.depth[base + i]; return; }
    float d, s;
    if (p.start_depth) { d = p.start_depth[base + i]; s = p.start_sigma[base + i]; }
    else if (!p.started[seq]) { d = a.depth[base + i]; s = a.sigma[base + i]; }
    else { d = p.init_depth[i]; s = p.init_sigma[i]; }
    int x, y;
    split_row(i, w, a.inv_w, x, y);
    const float g = p.frm_gray[T][base + i];
    p.ref_gray[T][base + i] = g;
    p.ring_gray[(size_t)seq * p.R * w * h + i] = g;
    a.depth_top_out[base + i] = d;
    p.sigma_top[base + i] = s;
    p.age[base + i] = 0.0f;
    a.wgt[T][base + i] = gn_weight(a.step[T], a.sigma_min, a.sigma_max, s);
    const float vd = pass_valid(d), vs = pass_valid(s);
    for (int t = 1; t < a.levels; t++) {
        const int msk = (1 << t) - 1;
        if ((x & msk) | (y & msk)) break;
        const int l = T - t, lx = x >> t, ly = y >> t;
        if (lx >= a.w[l] || ly >= a.h[l]) continue;
        const size_t o = (size_t)seq * a.w[l] * a.h[l] + (size_t)ly * a.w[l] + lx;
        p.ref_gray[l][o] = p.frm_gray[l][o];
        a.depth_lv[l][o] = vd;
        a.sigma_lv[l][o] = vs;
        a.wgt[l][o] = gn_weight(a.step[l], a.sigma_min, a.sigma_max, vs);
    }
}

// ------------------------------------------------------------------------------------------------
// One reference pixel of Mapper::update + Implement::update (mapper.cpp:76-137, implement.cpp:23-152,182-214).  The per-keyframe
// relative poses come from k_age_table (never a per-pixel exp/log).  Split in a head (up to the epipolar segment, which fixes the
// number of search steps) and a tail (the search and what follows), so that k_depth_update can reorder pixels between the two.
// GlobalImg (dvo_math.h) with the address space stated: a keyframe image reached through a pointer table is otherwise a flat pointer
struct GlobalImgG {
    const __attribute__((address_space(1))) float* p;
    int w, h;
    __device__ __forceinline__ float at(int x, int y) const { return p[y * w + x]; }
};

struct UpdHead {   // what the head of the per-pixel computation hands to the search (kept in LDS between the two phases of k_depth_update)
    float sx, sy, ex, ey, length, depth, sigma, dmin, dmax;
    int qx, qy, bi;
};

// Head: mapper.cpp:90-107 + EpipolarSegment (implement.cpp:23-47).  Returns the number of search steps the pixel will take
// (an upper bound within one step; 0 = the pixel leaves before the search: nothing to do).
// PCAM: the sequence's intrinsics `cam` instead of a.k (map_intr).
template <bool PCAM>
__device__ __forceinline__ int depth_update_head(const UpdateArgs& a, const int seq, const int x, const int y, UpdHead& hd, const Intr& cam)
{
    const int w = a.w, h = a.h, npix = w * h;
    const MonoSeq* m = a.meta ? a.meta + seq : nullptr;
    const int i = y * w + x;
    const size_t base = (size_t)seq * npix;
    const Pose rel_pose = m ? m->rel_pose : a.rel_pose;
    const float rel_tz = m ? m->rel_xi[2] : a.rel_tz;
    int n_hist = a.n_hist;
    if (m && a.ring_gray) n_hist = m->n_total < a.R ? m->n_total : a.R;
    const float d = a.ref_depth[base + i];
    float pu, pv;
    warp(rel_pose, map_intr<PCAM>(a, cam), (float)x, (float)y, d, pu, pv);   // mapper.cpp:94
    int qx, qy;
    if (!round_coord(pu, qx) || !round_coord(pv, qy)) return 0;
    if (qx < 0 || w <= qx || qy < 0 || h <= qy) return 0;
    const int age = (int)a.ref_age[base + i];                          // mapper.cpp:99
    int bi = n_hist - 1 - age;                                         // frame.hpp:176
    if (bi < 0 && a.clamp_age) {   // (rare: only once a sequence has created more than R keyframes and a pixel survived them all)
        bi = 0;
        if (m) atomicAdd(const_cast<int*>(&m->clamped), 1);
    }
    if (bi < 0 || bi >= n_hist) return 0;
    const AgeEntry& born = a.ages[(size_t)seq * a.R + bi];
    const float depth = d - rel_tz;                                    // mapper.cpp:104
    const float sigma = a.ref_sigma[base + i];
    // EpipolarSegment, implement.cpp:23-47
    const float dmin = (depth - sigma) < 0.10f ? 0.10f : (depth - sigma);
    const float dmax = depth + sigma;
    float sx, sy, ex, ey;
    warp(born.pose, map_intr<PCAM>(a, cam), (float)qx, (float)qy, dmax, sx, sy);
    warp(born.pose, map_intr<PCAM>(a, cam), (float)qx, (float)qy, dmin, ex, ey);
    const float sex = sx - ex, sey = sy - ey;
    const float length = (float)sqrt((double)sex * (double)sex + (double)sey * (double)sey);
    hd.sx = sx; hd.sy = sy; hd.ex = ex; hd.ey = ey; hd.length = length; hd.depth = depth; hd.sigma = sigma; hd.dmin = dmin; hd.dmax = dmax;
    hd.qx = qx; hd.qy = qy; hd.bi = bi;
    // steps of the search loop: it runs while |pt - start| < length, pt advancing one pixel per step, at most 102 times
    if (!(length > 0.0f)) return 1;                       // (NaN or zero length: the loop test fails at once; the pixel still has its tail)
    return length >= 102.0f ? 103 : (int)length + 2;
}

// Tail: doMatching, depthEstimate, sigmaEstimate and the fusion (implement.cpp:49-152,182-214, mapper.cpp:122-131) of one pixel.
// PCAM: the sequence's intrinsics `cam` and culled K9 / k_sparse `mk` instead of a.k, a.K9 and a.k_sparse.
template <bool PCAM>
__device__ __forceinline__ void depth_update_tail(const UpdateArgs& a, const int seq, const int x, const int y, const UpdHead& hd, const Intr& cam,
                                                  const MapK& mk)
{
    const int w = a.w, h = a.h, npix = w * h;
    const MonoSeq* m = a.meta ? a.meta + seq : nullptr;
    const int i = y * w + x;
    const size_t base = (size_t)seq * npix;
    const int obj_id = m ? m->frame_id : a.obj_id;
    const AgeEntry& born = a.ages[(size_t)seq * a.R + hd.bi];
    const float* born_gray = a.ring_gray ? a.ring_gray + ((size_t)seq * a.R + born.slot) * npix : a.gray_table[born.slot];
    const GlobalImgG bg{(const __attribute__((address_space(1))) float*)born_gray, w, h};
    const float sx = hd.sx, sy = hd.sy, ex = hd.ex, ey = hd.ey, length = hd.length, depth = hd.depth, sigma = hd.sigma, dmin = hd.dmin, dmax = hd.dmax;
    const int qx = hd.qx, qy = hd.qy;
    const float sex = sx - ex, sey = sy - ey;
    // doMatching, implement.cpp:106-152
    const float og = a.obj_gray[base + qy * w + qx];
    const float dirx = (ex - sx) / length, diry = (ey - sy) / length;
    float ptx = sx, pty = sy, bestx = sx, besty = sy, min_ssd = 6.0f;
    float s_c = 0.0f, s_pc = 0.0f, pcx = 0.0f, pcy = 0.0f;   // sample reuse between steps (see the loop)
    int count = 0;
    // The loop test of implement.cpp:113 is sqrt(dx^2 + dy^2) < length in double.  With L2 = length^2 (exact in double), that is
    // decided without the square root whenever dx^2 + dy^2 is not within a relative 1e-12 of L2 (sqrt is monotonic and correctly
    // rounded: its result can only differ from the exact root's side of `length` inside that band); inside the band the literal
    // test runs.  Same decisions, one fp64 sqrt per pixel instead of one per step.
    const double Ld = (double)length, L2 = Ld * Ld, L2lo = L2 * (1.0 - 1e-12), L2hi = L2 * (1.0 + 1e-12);
    // ... and a float estimate of dx^2 + dy^2 (relative error < 2e-7) decides every step that is not within 1e-5 of the end of the
    // segment without any fp64 instruction; the double test above only runs in that last sliver (and for NaN / overflow).
    const float L2f = length * length, L2f_lo = L2f * (1.0f - 1e-5f), L2f_hi = L2f * (1.0f + 1e-5f);
    for (;;) {
        const float ddx = ptx - sx, ddy = pty - sy;
        const float q2f = fmaf(ddx, ddx, ddy * ddy);
        bool go;
        if (q2f < L2f_lo) go = true;
        else if (q2f > L2f_hi) go = false;
        else {
            const double q2 = (double)ddx * (double)ddx + (double)ddy * (double)ddy;
            if (q2 < L2lo) go = true;
            else if (q2 > L2hi) go = false;
            else go = sqrt(q2) < Ld;              // (also the NaN case: every comparison above is false)
        }
        if (!go) break;
        float ssd = 0.0f;
        ptx += dirx;
        pty += diry;
        // A step samples at pt - dir, pt and pt + dir (implement.cpp:124-126: pt + (i - N/2) * dir, i = 0, 1, 2).  pt + dir is, bit for
        // bit, the NEXT step's pt (the same float addition), so that sample is computed once and is the next step's centre; and
        // pt - dir equals the PREVIOUS step's pt except where the addition rounded across a binade (checked per step and lane, in
        // both coordinates): then the previous centre sample is this step's first.  Same coordinates -> same taps, fractions and
        // blend -> the same sample values as three evaluations per step, for ~1.3 evaluations (one new sample, plus the first one
        // again for the whole wave when any lane's round trip failed).  The first step of a pixel evaluates all three.
        // The reference's early exit -- the first INVALID sample sets ssd = 6 and leaves (implement.cpp:128-131) -- is applied to
        // the values: same result.
        float sgv[3];
        const float nx = ptx + dirx * -1.0f, ny = pty + diry * -1.0f;   // (the literal expressions of the three targets)
        const float cx = ptx + dirx * 0.0f, cy = pty + diry * 0.0f;
        const float fx = ptx + dirx * 1.0f, fy = pty + diry * 1.0f;
        const bool first = count == 0;                                     // wave-uniform: the lanes of a wave enter the loop together
        // (cx, cy) == the previous step's (fx, fy) holds by construction from the second step on (cx = pt + 0*dir = pt for finite dir;
        //  for a non-finite dir every sample of every step is INVALID either way)
        const bool need_n = first | !((nx == pcx) & (ny == pcy));
        const bool any_n = __ballot(need_n) != 0ull;
        // Interior fast path: pt in [2, w-3) x [2, h-3) and |dir| <= 1 (+ an ulp) put all three samples' 2 x 2 footprints inside the
        // image, where Convert::getSubpixelFromDense (convert.cpp:77-105) has no clamp, no range test and no INVALID exit: the same
        // truncation, fractions and blend4() without ~20 instructions of bounds logic per sample.  Wave-uniform choice.
        const bool inner = (ptx >= 2.0f) & (ptx < (float)(w - 3)) & (pty >= 2.0f) & (pty < (float)(h - 3));
        float s_n = s_pc, s_f;
        if (__ballot(!inner) == 0ull) {
            auto fast = [&](float px, float py) {
                const int x0 = (int)px, y0 = (int)py;
                // (global address space stated: born_gray may come from a pointer table, which makes it a flat pointer -- and flat loads
                //  also count against lgkmcnt and take the aperture check)
                const __attribute__((address_space(1))) float* q = (const __attribute__((address_space(1))) float*)born_gray + (y0 * w + x0);
                return blend4(q[0], q[1], q[w], q[w + 1], px - (float)x0, py - (float)y0);
            };
            s_f = fast(fx, fy);
            if (first) s_c = fast(cx, cy);
            if (any_n) { const float t = fast(nx, ny); s_n = need_n ? t : s_pc; }
        } else {
            s_f = get_subpixel_dense(bg, fx, fy);
            if (first) s_c = get_subpixel_dense(bg, cx, cy);
            if (any_n) { const float t = get_subpixel_dense(bg, nx, ny); s_n = need_n ? t : s_pc; }
        }
        sgv[0] = s_n; sgv[1] = s_c; sgv[2] = s_f;
        s_pc = s_c; pcx = cx; pcy = cy;      // this step's centre: the next step's first sample where the round trip holds
        s_c = s_f;                           // this step's far sample: the next step's centre
        bool any_invalid = false;
#pragma unroll
        for (int jj = 0; jj < 3; jj++) {
            any_invalid = any_invalid | is_invalid(sgv[jj]);
            const float diff = sgv[jj] - og;
            const int aw = 3 - abs(jj - 2);
            ssd = (float)((double)ssd + 1.0 * aw / 3 * (double)(diff * diff));  // implement.cpp:134 (discarded when a sample is INVALID)
        }
        if (any_invalid) ssd = 6.0f;
        if (ssd < min_ssd) { bestx = ptx; besty = pty; min_ssd = ssd; }
        if (count++ > 100) break;
    }
    if ((double)min_ssd > 3 * 0.1) return;                             // implement.cpp:145
    if (bestx < 0.0f || besty < 0.0f || bestx > (float)w || besty > (float)h) return;  // implement.cpp:196-200
    // depthEstimate, implement.cpp:49-71 (double from float inputs)
    float nd;
    {
        float q0f, q1f, q2f;
        back_project(map_intr<PCAM>(a, cam), (float)qx, (float)qy, 1.0f, q0f, q1f, q2f);
        const double q0 = q0f, q1 = q1f, q2 = q2f;
        const double t[3] = {(double)born.tneg[0], (double)born.tneg[1], (double)born.tneg[2]};
        const double xi3[3] = {(double)bestx, (double)besty, 1.0};
        double Rq[3], KRq[3], Kt[3];
        for (int r = 0; r < 3; r++)
            Rq[r] = (double)born.pose.R[3 * r] * q0 + (double)born.pose.R[3 * r + 1] * q1 + (double)born.pose.R[3 * r + 2] * q2;
        const float* K9 = PCAM ? mk.K9 : a.K9;
        const int k_sparse = PCAM ? mk.k_sparse : a.k_sparse;
        if (k_sparse) {
            // K = [fx 0 cx; 0 fy cy; 0 0 1]: a product with an exact zero adds an exact zero, so (fx x + 0 y) + cx z is fx x + cx z and
            // (0 x + 0 y) + 1 z is z -- the same doubles as the three-term rows below (for finite x, y, z: they are), 12 instead of 30
            // fp64 operations per pixel for K R q and K t.
            const double fx = (double)K9[0], cx = (double)K9[2], fy = (double)K9[4], cy = (double)K9[5];
            KRq[0] = fx * Rq[0] + cx * Rq[2]; KRq[1] = fy * Rq[1] + cy * Rq[2]; KRq[2] = Rq[2];
            Kt[0] = fx * t[0] + cx * t[2]; Kt[1] = fy * t[1] + cy * t[2]; Kt[2] = t[2];
        } else {
            for (int r = 0; r < 3; r++) {
                KRq[r] = (double)K9[3 * r] * Rq[0] + (double)K9[3 * r + 1] * Rq[1] + (double)K9[3 * r + 2] * Rq[2];
                Kt[r] = (double)K9[3 * r] * t[0] + (double)K9[3 * r + 1] * t[1] + (double)K9[3 * r + 2] * t[2];
            }
        }
        double aa = 0.0, ab = 0.0;
        // (sparse K: the third components are Rq[2] * 1 - Rq[2] and t[2] * 1 - t[2], exact zeros whose products add exact zeros)
        const int nr = k_sparse ? 2 : 3;
        for (int r = 0; r < nr; r++) {
            const double va = Rq[2] * xi3[r] - KRq[r];
            const double vb = t[2] * xi3[r] - Kt[r];
            aa += va * va;
            ab += va * vb;
        }
        nd = -(float)(ab / aa);
    }
    // sigmaEstimate, implement.cpp:73-104
    float ns;
    {
        const float l = length;
        const float lx = sex / l, ly = sey / l;
        const float alpha = (dmax - dmin) / l;
        int mx = 0, my = 0;
        round_coord(bestx, mx);
        round_coord(besty, my);
        mx = mx < 0 ? 0 : (mx > w - 1 ? w - 1 : mx);  // D5 clamp
        my = my < 0 ? 0 : (my > h - 1 ? h - 1 : my);
        const float gx = grad_x_at(bg, mx, my), gy = grad_y_at(bg, mx, my);
        if (is_invalid(gx) || is_invalid(gy)) return;  // new_sigma = -1 fails the gate of mapper.cpp:122
        const float gl = fabsf(fmaf(gy, ly, gx * lx));
        const float gl2 = gl * gl, gp2 = gl / l;
        const float epi = 0.25f / (gl2 < kEpsilon ? kEpsilon : gl2);
        const float lum = 0.5f / (gp2 < kEpsilon ? kEpsilon : gp2);
        ns = alpha * sqrtf(epi + lum);
    }
    if (nd > 0.2f && nd < 6.0f && ns > 0.0f && ns < 0.5f) {            // mapper.cpp:122
        float gd = depth, gs = sigma;
        const float reset = rng_depth(a.seed, (uint32_t)obj_id, (uint32_t)i);
        if (!gaussian_update(gd, gs, nd, ns, reset)) a.ref_age[base + i] = 0.0f;  // mapper.cpp:124-127
        else atomicAdd(a.valid_updates ? a.valid_updates : const_cast<int*>(&m->valid_updates), 1);   // (an explicit counter wins)
        a.ref_depth[base + i] = gd;                                    // mapper.cpp:130-131
        a.ref_sigma[base + i] = gs;
    }
}

// Mapper::update + Implement::update (mapper.cpp:76-137, implement.cpp:23-152,182-214): one thread per reference pixel of the
// window mapper.cpp:90 keeps.  FP32-VALU bound (<= 102 search steps x 3 bilinear samples per pixel), not HBM bound.
// The search length varies per pixel by two orders of magnitude (it is the epipolar segment of depth +- sigma: a few pixels for most,
// ~100 where depth - sigma clamps at 0.10 m) and a wave runs as long as its longest lane.  So the workgroup first computes every
// pixel's step count (the cheap head of the computation), sorts its 256 pixels by it (counting sort in LDS, longest first) and
// hands them out in that order: each wave then holds pixels of similar length and finishes together.  Pixels that leave before
// the search are dropped from the list.  Pixels are independent and the valid-update count is an integer sum, so the order changes
// no result (bit-exact vs the oracle and the one-pass form: tests/test_gpu_parity.py, tests/test_real_data.py).
// PCAM (k_depth_update_cam): per-sequence intrinsics (UpdateArgs::seq_k, seq_K9), loaded once per workgroup into SGPRs.  The
// arguments are taken by value, as in propagate_owner.
template <bool PCAM>
__device__ __forceinline__ void depth_update(UpdateArgs a)
{
    __shared__ int bucket_cnt[128];     // pixels per step count, index 127 - steps (longest first)
    __shared__ int bucket_off[128];
    __shared__ int order[256];          // producer thread of the pixel each thread searches
    __shared__ int n_listed;
    __shared__ float head_f[9][256];    // UpdHead of every listed pixel, by producer thread (the head is computed once)
    __shared__ int head_i[3][256];
    const int w = a.w, h = a.h;
    // Only the window of mapper.cpp:90 (x in [16,144], y in [12,108]) is launched when the crop is on.
    const int x_lo = a.crop ? 16 : 0, y_lo = a.crop ? 12 : 0;
    const int ww = a.crop ? (min(144, w - 1) - 16 + 1) : w, wh = a.crop ? (min(108, h - 1) - 12 + 1) : h;
    if (ww <= 0 || wh <= 0) return;
    int seq, j;
    const bool mine = seq_pixel(ww * wh, a.n_seq, seq, j);       // (seq is block-uniform; only the last block of a sequence has idle threads)
    if (seq >= a.n_seq) return;
    if (a.meta && a.ring_gray && a.meta[seq].need) return;   // this sequence created a keyframe instead (mapper.cpp:23-27); block-uniform
    Intr cam;
    MapK mk;
    if constexpr (PCAM) { cam = load_seq_entry(a.seq_k, seq); mk = load_seq_entry(a.seq_K9, seq); }
    const int j0 = j - (int)threadIdx.x;                 // window index of this workgroup's first thread
    if (threadIdx.x < 128) bucket_cnt[threadIdx.x] = 0;
    __syncthreads();
    int steps = 0, rank = 0;
    if (mine) {
        int wx, wy;
        split_row(j, ww, a.inv_ww, wx, wy);
        UpdHead hd;
        steps = depth_update_head<PCAM>(a, seq, x_lo + wx, y_lo + wy, hd, cam);
        if (steps > 0) {
            rank = atomicAdd(&bucket_cnt[127 - steps], 1);
            const int t = (int)threadIdx.x;
            head_f[0][t] = hd.sx; head_f[1][t] = hd.sy; head_f[2][t] = hd.ex; head_f[3][t] = hd.ey; head_f[4][t] = hd.length;
            head_f[5][t] = hd.depth; head_f[6][t] = hd.sigma; head_f[7][t] = hd.dmin; head_f[8][t] = hd.dmax;
            head_i[0][t] = hd.qx; head_i[1][t] = hd.qy; head_i[2][t] = hd.bi;
        }
    }
    __syncthreads();
    if (threadIdx.x < 64) {   // exclusive prefix sum over the 128 buckets, two per lane of wave 0
        const int b0 = 2 * (int)threadIdx.x;
        const int c0 = bucket_cnt[b0], c1 = bucket_cnt[b0 + 1];
        int incl = c0 + c1;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d);
            if ((int)threadIdx.x >= d) incl += up;
        }
        const int excl = incl - (c0 + c1);
        bucket_off[b0] = excl;
        bucket_off[b0 + 1] = excl + c0;
        if (threadIdx.x == 63) n_listed = incl;
    }
    __syncthreads();
    if (steps > 0) order[bucket_off[127 - steps] + rank] = (int)threadIdx.x;
    __syncthreads();
    if ((int)threadIdx.x < n_listed) {
        const int p = order[threadIdx.x];
        UpdHead hd;
        hd.sx = head_f[0][p]; hd.sy = head_f[1][p]; hd.ex = head_f[2][p]; hd.ey = head_f[3][p]; hd.length = head_f[4][p];
        hd.depth = head_f[5][p]; hd.sigma = head_f[6][p]; hd.dmin = head_f[7][p]; hd.dmax = head_f[8][p];
        hd.qx = head_i[0][p]; hd.qy = head_i[1][p]; hd.bi = head_i[2][p];
        const int jq = j0 + p;
        int wx, wy;
        split_row(jq, ww, a.inv_ww, wx, wy);
        depth_update_tail<PCAM>(a, seq, x_lo + wx, y_lo + wy, hd, cam, mk);
    }
}

__global__ void __launch_bounds__(256) k_depth_update(UpdateArgs a) { depth_update<false>(a); }
__global__ void __launch_bounds__(256) k_depth_update_cam(UpdateArgs a) { depth_update<true>(a); }

// ------------------------------------------------------------------------------------------------
// k_promote: the tracked frame becomes the newest keyframe (Mapper::estimate's needNewFrame branch, mapper.cpp:23-27 +
// FrameHistory::push): its gray pyramid, the propagated top-level depth / sigma and the age map are copied over the reference
// set's, and its top-level gray enters the keyframe ring (slot n_total % R).  One launch, every segment of every flagged sequence.
// ------------------------------------------------------------------------------------------------
#define DVO_PROMOTE_PER_THREAD 8
// VEC = 4: every segment length is a multiple of 4 floats (the usual geometries), copied as 16-byte accesses; VEC = 1: any length
template <int VEC>
__global__ void __launch_bounds__(256) k_promote(PromoteArgs a)
{
    typedef float fvec __attribute__((ext_vector_type(VEC)));
    int total = a.npix;  // + the ring segment
    for (int g = 0; g < a.n_seg; g++) total += a.count[g];
    total /= VEC;        // in units of VEC floats
    // 2048 units per workgroup: most sequences do not create a keyframe on a given frame, and a workgroup that only finds that
    // out costs as much to dispatch as one that copies -- fewer, fatter workgroups
    int seq, cursor = -1;
    const int i0 = (int)blockIdx.x * (256 * DVO_PROMOTE_PER_THREAD) + (int)threadIdx.x;
    while (next_listed_seq(a.all ? nullptr : a.need_list, a.n_slots, a.n_seq, a.all ? nullptr : a.meta, cursor, seq)) {
        const MonoSeq& m = a.meta[seq];
        const int slot = a.all ? 0 : m.n_total % a.R;   // (k_mono_commit increments n_total AFTER this kernel)
#pragma unroll
        for (int k = 0; k < DVO_PROMOTE_PER_THREAD; k++) {
            int i = i0 + k * 256;
            if (i >= total) break;
            bool done = false;
            for (int g = 0; g < a.n_seg; g++) {
                const int cnt = a.count[g] / VEC;
                if (i < cnt) {
                    const size_t o = (size_t)seq * cnt + i;
                    reinterpret_cast<fvec*>(a.dst[g])[o] = reinterpret_cast<const fvec*>(a.src[g])[o];
                    done = true;
                    break;
                }
                i -= cnt;
            }
            if (!done) {
                const int cnt = a.npix / VEC;
                reinterpret_cast<fvec*>(a.ring_gray)[((size_t)seq * a.R + slot) * cnt + i] = reinterpret_cast<const fvec*>(a.gray_top)[(size_t)seq * cnt + i];
            }
        }
    }
}

__global__ void __launch_bounds__(256) k_broadcast(const float* __restrict__ src, float* __restrict__ dst, int count, int n_seq)
{
    int seq, i;
    if (!seq_pixel(count, n_seq, seq, i)) return;
    dst[(size_t)seq * count + i] = src[i];
}

// ------------------------------------------------------------------------------------------------
// Keyframe depth fusion and keyframe carry of a sensor-depth batch (dvo_batch_set_keyframe_fusion, dvo_batch_set_keyframe_carry; the
// contracts are in include/dvo.h).  Both work on a lane's own four pixels of one map in place and gather
// from the other map through the push's relative pose; what they share is below, what each keeps for itself is at its kernel.
// Prep (one thread per sequence): what k_kf_decide left of the push as one table entry -- F = MonoSeq::rel_pose = float(exp(+xi)),
// Bk = float(exp(-xi)) through the same double-precision chain, for a TRACK sequence with a finite twist that the kernel works on --
// and the sequence's record zeroed.  k_kf_decide itself is not touched.
//   k_kf_fuse_prep:  clear (a start or a promotion), fuse (TRACK, rule not fired) or nothing.
//   k_kf_carry_prep: carry (TRACK, rule fired) or nothing.
// ------------------------------------------------------------------------------------------------
template <bool CARRY>
__device__ __forceinline__ void kf_prep(KfPrepArgs a)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= a.n_seq) return;
    const MonoSeq& m = a.meta[s];
    const int eff = a.eff[s];
    const bool track = eff == DVO_SEQ_TRACK;
    KfSeq e;
    for (int i = 0; i < 9; i++) { e.F.R[i] = 0.0f; e.Bk.R[i] = 0.0f; }
    for (int i = 0; i < 3; i++) { e.F.t[i] = 0.0f; e.Bk.t[i] = 0.0f; e.pad[i] = 0; }
    e.mode = CARRY ? DVO_KF_CARRY_NONE : DVO_KF_FUSE_NONE;
    if (!CARRY && (eff == DVO_SEQ_RESTART || (track && a.is_key[s]))) {
        e.mode = DVO_KF_FUSE_CLEAR;
    } else if (track && (!CARRY || a.is_key[s])) {
        float xi[6];
        bool finite = true;
        for (int i = 0; i < 6; i++) { xi[i] = m.rel_xi[i]; finite = finite && isfinite(xi[i]); }
        if (finite) {
            e.mode = CARRY ? DVO_KF_CARRY_CARRY : DVO_KF_FUSE_FUSE;
            e.F = m.rel_pose;
            pose_from_xi(xi, -1.0f, e.Bk);
        }
    }
    a.table[s] = e;
    KfRecord z;
    z.n_candidates = 0; z.n_done = 0; z.n_gated = 0; z.pad = 0;
    a.rec[s] = z;
}

__global__ void __launch_bounds__(64) k_kf_fuse_prep(KfPrepArgs a) { kf_prep<false>(a); }
__global__ void __launch_bounds__(64) k_kf_carry_prep(KfPrepArgs a) { kf_prep<true>(a); }

// A lane: four consecutive top-level pixels, the plane addressed linearly (a sequence's plane starts on a 4-byte boundary only: the
// 16-byte, 8-byte and 4-byte accesses are declared unaligned); the last lane of a plane whose size is no multiple of 4 goes pixel by
// pixel.  No float atomics, no LDS.
typedef float kf_f4 __attribute__((ext_vector_type(4), aligned(4)));
typedef float kf_f2 __attribute__((ext_vector_type(2), aligned(4)));
typedef uint32_t kf_u32 __attribute__((aligned(1)));
#define DVO_KF_FUSE_PER_THREAD 4

struct KfLane {
    int first, nk;   // the lane's first pixel (0 for a lane past the plane) and how many it has
    bool full;
    size_t base;     // the sequence's plane
    int x, y;        // (column, row) of `first`
};
__device__ __forceinline__ KfLane kf_lane(int seq, int w, int h, float inv_w)
{
    const int n = w * h;
    const int i0 = ((int)blockIdx.x * 256 + (int)threadIdx.x) * DVO_KF_FUSE_PER_THREAD;
    KfLane L;
    L.nk = i0 >= n ? 0 : (n - i0 < DVO_KF_FUSE_PER_THREAD ? n - i0 : DVO_KF_FUSE_PER_THREAD);
    L.first = L.nk ? i0 : 0;
    L.full = L.nk == DVO_KF_FUSE_PER_THREAD;
    L.base = (size_t)seq * n;
    split_row(L.first, w, inv_w, L.x, L.y);
    return L;
}
// The lane's pixels at p and their count bytes at cb, packed into c4: a pixel the lane does not have reads as 0 and is not written.
// Either pointer may be null (a constant at every call): that half is left out.
__device__ __forceinline__ void kf_load_lane(const KfLane& L, const float* p, const uint8_t* cb, float d[DVO_KF_FUSE_PER_THREAD], uint32_t& c4)
{
    for (int k = 0; k < DVO_KF_FUSE_PER_THREAD; k++) d[k] = 0.0f;
    c4 = 0;
    if (L.full) {
        const kf_f4 v = *reinterpret_cast<const kf_f4*>(p);
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        if (cb) c4 = *reinterpret_cast<const kf_u32*>(cb);
    } else {
        for (int k = 0; k < L.nk; k++) {
            d[k] = p[k];
            if (cb) c4 |= (uint32_t)cb[k] << (8 * k);
        }
    }
}
__device__ __forceinline__ void kf_store_lane(const KfLane& L, float* p, const float* d, uint8_t* cb, uint32_t c4)
{
    if (L.full) {
        if (p) {
            kf_f4 v;
            v.x = d[0]; v.y = d[1]; v.z = d[2]; v.w = d[3];
            *reinterpret_cast<kf_f4*>(p) = v;
        }
        if (cb) *reinterpret_cast<kf_u32*>(cb) = c4;
    } else {
        for (int k = 0; k < L.nk; k++) {
            if (p) p[k] = d[k];
            if (cb) cb[k] = (uint8_t)(c4 >> (8 * k));
        }
    }
}

// Pixel (x, y) of one map at depth dk, through pose `go` into the other map's top-level plane `other` and back through pose `back`:
// KF_MISS when it lands behind min_depth or outside the plane, or a tap is below min_depth, not finite, or the four spread more than
// max_diff; KF_GATED when the bilinear depth there disagrees with the warped point's by more than max_diff; KF_MISS again when the
// point that comes back is out of range; else KF_HIT with zr = its depth back in the pixel's own map and o = the offset of the first
// tap within the plane (a plane has fewer than 2^24 pixels: split_row).  PAIRED: the taps are two 8-byte loads, not four 4-byte ones
// (each caller keeps the loads it was measured with).
enum { KF_MISS = 0, KF_GATED = 1, KF_HIT = 2 };
template <bool PCAM, bool PAIRED, class Args>
__device__ __forceinline__ int kf_warp_gate(const Args& a, const Intr& cam, const Pose& go, const Pose& back, const float* __restrict__ other,
                                            int w, int h, int x, int y, float dk, float& zr, int& o)
{
    const float md = a.min_depth, inf = __builtin_inff();
    float X, Y, Z, Xg, Yg, Zg;
    back_project(map_intr<PCAM>(a, cam), (float)x, (float)y, dk, X, Y, Z);
    transform(go, X, Y, Z, Xg, Yg, Zg);
    if (!(Zg >= md)) return KF_MISS;
    float u, v;
    project(map_intr<PCAM>(a, cam), Xg, Yg, Zg, u, v);
    if (!(u >= 0.0f && u < (float)(w - 1) && v >= 0.0f && v < (float)(h - 1))) return KF_MISS;
    const int x0 = (int)u, y0 = (int)v;
    const float fa = u - (float)x0, fb = v - (float)y0;
    o = y0 * w + x0;
    float z00, z10, z01, z11;
    if constexpr (PAIRED) {
        const kf_f2 r0 = *reinterpret_cast<const kf_f2*>(other + o), r1 = *reinterpret_cast<const kf_f2*>(other + o + w);
        z00 = r0.x; z10 = r0.y; z01 = r1.x; z11 = r1.y;
    } else {
        const float* p = other + o;
        z00 = p[0]; z10 = p[1]; z01 = p[w]; z11 = p[w + 1];
    }
    bool ok = (z00 >= md) & (z00 < inf) & (z10 >= md) & (z10 < inf) & (z01 >= md) & (z01 < inf) & (z11 >= md) & (z11 < inf);
    const float mx = fmaxf(fmaxf(z00, z10), fmaxf(z01, z11)), mn = fminf(fminf(z00, z10), fminf(z01, z11));
    ok = ok && (mx - mn <= a.max_diff);
    if (!ok) return KF_MISS;
    const float top = fmaf(fa, z10 - z00, z00), bot = fmaf(fa, z11 - z01, z01);
    const float zi = fmaf(fb, bot - top, top);
    if (!(fabsf(zi - Zg) <= a.max_diff)) return KF_GATED;
    float Xb, Yb;
    back_project(map_intr<PCAM>(a, cam), u, v, zi, X, Y, Z);
    transform(back, X, Y, Z, Xb, Yb, zr);
    return (zr >= md && zr < inf) ? KF_HIT : KF_MISS;
}

// dn at top-level pixel (x, y) into the lower levels of `pyr`: they keep the pixels whose coordinates are multiples of 2^t
template <class Args>
__device__ __forceinline__ void kf_write_lower(const Args& a, float* const* pyr, int seq, int x, int y, float dn)
{
    const int T = a.levels - 1;
    for (int t = 1; t < a.levels; t++) {
        const int msk = (1 << t) - 1;
        if ((x & msk) | (y & msk)) break;
        const int l = T - t, lx = x >> t, ly = y >> t;
        if (lx >= a.w[l] || ly >= a.h[l]) continue;
        pyr[l][(size_t)seq * a.w[l] * a.h[l] + (size_t)ly * a.w[l] + lx] = dn;
    }
}

// A lane's tally is candidates | done << 10 | gated << 20 (at most 4 of each per lane, 256 per wave): summed per wave by one packed
// butterfly (every lane of the wave must be here) and added to the sequence's record with integer atomics: order-free.
#define DVO_KF_TALLY_DONE  (1 << 10)
#define DVO_KF_TALLY_GATED (1 << 20)
__device__ __forceinline__ void kf_tally(int tally, KfRecord* r)
{
    for (int o = 32; o > 0; o >>= 1) tally += __shfl_xor(tally, o);
    if ((threadIdx.x & 63) == 0) {
        if (tally & 0x3ff) atomicAdd(&r->n_candidates, tally & 0x3ff);
        if ((tally >> 10) & 0x3ff) atomicAdd(&r->n_done, (tally >> 10) & 0x3ff);
        if ((tally >> 20) & 0x3ff) atomicAdd(&r->n_gated, (tally >> 20) & 0x3ff);
    }
}

// k_kf_fuse: the lane's pixels are the keyframe's, read and written in place with their own counts; it goes through F, gathers four
// scalar taps from the tracked frame's map (which nobody writes) and comes back through Bk.  Its own: the clear mode; a candidate is
// any depth >= min_depth; the count is the pixel's own byte; the blend moves 1 / (c + 2) of the way to the returned depth; depth and
// counts go back only from a lane that fused something.
template <bool PCAM>
__device__ __forceinline__ void kf_fuse(KfFuseArgs a)
{
    const int seq = grid_seq();
    if (seq >= a.n_seq) return;
    const KfSeq e = load_seq_entry(a.table, seq);   // uniform per workgroup: scalar loads
    if (e.mode == DVO_KF_FUSE_NONE) return;
    const int T = a.levels - 1, w = a.w[T], h = a.h[T];
    const KfLane L = kf_lane(seq, w, h, a.inv_w);
    uint8_t* cnt = a.counts + L.base + L.first;
    if (e.mode == DVO_KF_FUSE_CLEAR) { kf_store_lane(L, nullptr, nullptr, cnt, 0u); return; }
    Intr cam;
    if constexpr (PCAM) cam = load_seq_entry(a.seq_k, seq);
    float* kd = a.kf_depth[T] + L.base + L.first;
    float d[DVO_KF_FUSE_PER_THREAD];
    uint32_t c4;
    kf_load_lane(L, kd, cnt, d, c4);
    int x = L.x, y = L.y, tally = 0;
#pragma unroll
    for (int k = 0; k < DVO_KF_FUSE_PER_THREAD; k++) {
        const float dk = d[k];
        if (k < L.nk && dk >= a.min_depth) {
            float Zo;
            int o;
            const int g = kf_warp_gate<PCAM, false>(a, cam, e.F, e.Bk, a.frame_depth + L.base, w, h, x, y, dk, Zo, o);
            tally += 1;
            if (g == KF_GATED) tally += DVO_KF_TALLY_GATED;
            if (g == KF_HIT) {
                const int c = (int)((c4 >> (8 * k)) & 0xffu);
                const float dn = fmaf(Zo - dk, recip_rn((float)(c + 2)), dk);
                const int cn = c + 1 < a.max_count ? c + 1 : a.max_count;
                d[k] = dn;
                c4 = (c4 & ~(0xffu << (8 * k))) | ((uint32_t)cn << (8 * k));
                tally += DVO_KF_TALLY_DONE;
                kf_write_lower(a, a.kf_depth, seq, x, y, dn);
            }
        }
        x++;
        if (x == w) { x = 0; y++; }
    }
    if (tally & (0x3ff << 10)) kf_store_lane(L, kd, d, cnt, c4);
    kf_tally(tally, a.rec + seq);
}

__global__ void __launch_bounds__(256) k_kf_fuse(KfFuseArgs a) { kf_fuse<false>(a); }
__global__ void __launch_bounds__(256) k_kf_fuse_cam(KfFuseArgs a) { kf_fuse<true>(a); }

// k_kf_carry: the lane's pixels are the tracked frame's (the keyframe-to-be), read and written in place before k_promote copies
// them; it goes through Bk, gathers two 8-byte tap pairs from the old keyframe (which nobody writes during this launch) and comes back
// through F.  Its own: a candidate must also be finite; the count is the minimum of the four tap bytes (the old map stands for c + 1
// samples, the pixel's own for one: the blend moves (c + 1) / (c + 2) of the way); the blended depth must itself be in range; and,
// because neighbouring lanes gather the old counts, the new counts go to a staging plane -- every pixel of a carrying sequence, 0 where
// nothing was carried -- that k_kf_carry_commit copies after k_kf_fuse has cleared.
template <bool PCAM>
__device__ __forceinline__ void kf_carry(KfCarryArgs a)
{
    const int seq = grid_seq();
    if (seq >= a.n_seq) return;
    const KfSeq e = load_seq_entry(a.table, seq);   // uniform per workgroup: scalar loads
    if (e.mode != DVO_KF_CARRY_CARRY) return;
    const int T = a.levels - 1, w = a.w[T], h = a.h[T];
    const KfLane L = kf_lane(seq, w, h, a.inv_w);
    Intr cam;
    if constexpr (PCAM) cam = load_seq_entry(a.seq_k, seq);
    float* fd = a.frame_depth[T] + L.base + L.first;
    uint8_t* st = a.staged + L.base + L.first;
    const uint8_t* __restrict__ kc = a.counts + L.base;
    float d[DVO_KF_FUSE_PER_THREAD];
    uint32_t c4;
    kf_load_lane(L, fd, nullptr, d, c4);
    const float md = a.min_depth, inf = __builtin_inff();
    int x = L.x, y = L.y, tally = 0;
#pragma unroll
    for (int k = 0; k < DVO_KF_FUSE_PER_THREAD; k++) {
        const float dk = d[k];
        if (k < L.nk && dk >= md && dk < inf) {
            float Zp;
            int o;
            const int g = kf_warp_gate<PCAM, true>(a, cam, e.Bk, e.F, a.kf_depth + L.base, w, h, x, y, dk, Zp, o);
            tally += 1;
            if (g == KF_GATED) tally += DVO_KF_TALLY_GATED;
            if (g == KF_HIT) {
                const int c00 = kc[o], c10 = kc[o + 1], c01 = kc[o + w], c11 = kc[o + w + 1];
                const int ca = c00 < c10 ? c00 : c10, cb = c01 < c11 ? c01 : c11;
                const int c = ca < cb ? ca : cb;
                const float dn = fmaf(Zp - dk, (float)(c + 1) * recip_rn((float)(c + 2)), dk);
                if (dn >= md && dn < inf) {
                    const int cn = c + 1 < a.max_count ? c + 1 : a.max_count;
                    d[k] = dn;
                    c4 |= (uint32_t)cn << (8 * k);
                    tally += DVO_KF_TALLY_DONE;
                    kf_write_lower(a, a.frame_depth, seq, x, y, dn);
                }
            }
        }
        x++;
        if (x == w) { x = 0; y++; }
    }
    // (the staged counts always, the pixels from a lane that carried something; a tail lane writes its pixels back either way)
    kf_store_lane(L, !L.full || (tally & (0x3ff << 10)) ? fd : nullptr, d, st, c4);
    kf_tally(tally, a.rec + seq);
}

__global__ void __launch_bounds__(256) k_kf_carry(KfCarryArgs a) { kf_carry<false>(a); }
__global__ void __launch_bounds__(256) k_kf_carry_cam(KfCarryArgs a) { kf_carry<true>(a); }

// k_kf_carry_commit: the staged counts of the carrying sequences over the count plane (which k_kf_fuse has just cleared), four bytes
// per lane, declared unaligned; the last lane of a plane whose size is no multiple of 4 goes byte by byte.
__global__ void __launch_bounds__(256) k_kf_carry_commit(KfCarryCommitArgs a)
{
    const int seq = grid_seq();
    if (seq >= a.n_seq) return;
    if (load_seq_entry(a.table, seq).mode != DVO_KF_CARRY_CARRY) return;   // uniform per workgroup
    const int n = a.npix;
    const int i0 = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 4;
    if (i0 >= n) return;
    const size_t o = (size_t)seq * n + i0;
    if (n - i0 >= 4) *reinterpret_cast<kf_u32*>(a.counts + o) = *reinterpret_cast<const kf_u32*>(a.staged + o);
    else for (int k = 0; k < n - i0; k++) a.counts[o + k] = a.staged[o + k];
}

// ------------------------------------------------------------------------------------------------
// Keyframe maps as compacted world-frame point clouds (dvo_batch_export_points; the contract is in include/dvo.h).
// Sequences in index order, raster order within a sequence: the order comes from ranks and prefix sums only.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_points_prep(PointsPrepArgs a)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= a.n_seq) return;
    const MonoSeq& m = a.meta[s];
    bool on = a.started ? a.started[s] != 0 : (a.started_by_total ? m.n_total > 0 : true);
    if (a.select_new) on = on && a.is_key[s] != 0;
    PointsSeq e;
    for (int i = 0; i < 9; i++) e.Wk.R[i] = (i % 4 == 0) ? 1.0f : 0.0f;
    for (int i = 0; i < 3; i++) { e.Wk.t[i] = 0.0f; e.pad[i] = 0; }
    e.on = on ? 1 : 0;
    if (on) {
        float xi[6];
        for (int i = 0; i < 6; i++) xi[i] = m.ref_xi[i];
        pose_from_xi(xi, -1.0f, e.Wk);
    }
    a.table[s] = e;
    a.seq_total[s] = 0u;
}

// The gates of a lane's four consecutive pixels i0 .. i0 + nk - 1 of sequence plane `base`, as a bit mask; d[] = their depths and
// (x, y) = the first pixel.  The planes move as 16-byte (counts: 4-byte) accesses declared unaligned, as k_kf_fuse's; the last lane
// of a plane whose size is no multiple of 4 goes pixel by pixel.
__device__ __forceinline__ uint32_t points_gates(const PointsArgs& a, size_t base, int i0, int nk, float d[DVO_POINTS_PER_THREAD], int& x, int& y)
{
    const size_t o = base + (size_t)(nk ? i0 : 0);
    float sg[DVO_POINTS_PER_THREAD] = {0.0f, 0.0f, 0.0f, 0.0f}, ag[DVO_POINTS_PER_THREAD] = {0.0f, 0.0f, 0.0f, 0.0f};
    uint32_t c4 = 0;
    for (int k = 0; k < DVO_POINTS_PER_THREAD; k++) d[k] = 0.0f;
    if (nk == DVO_POINTS_PER_THREAD) {
        const kf_f4 v = *reinterpret_cast<const kf_f4*>(a.depth + o);
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        if (a.gate_sigma) {
            const kf_f4 t = *reinterpret_cast<const kf_f4*>(a.sigma + o);
            sg[0] = t.x; sg[1] = t.y; sg[2] = t.z; sg[3] = t.w;
        }
        if (a.age) {
            const kf_f4 t = *reinterpret_cast<const kf_f4*>(a.age + o);
            ag[0] = t.x; ag[1] = t.y; ag[2] = t.z; ag[3] = t.w;
        }
        if (a.counts) c4 = *reinterpret_cast<const kf_u32*>(a.counts + o);
    } else {
        for (int k = 0; k < nk; k++) {
            d[k] = a.depth[o + k];
            if (a.gate_sigma) sg[k] = a.sigma[o + k];
            if (a.age) ag[k] = a.age[o + k];
            if (a.counts) c4 |= (uint32_t)a.counts[o + k] << (8 * k);
        }
    }
    split_row(nk ? i0 : 0, a.w, a.inv_w, x, y);
    const int st = a.stride;
    int xx = x, xm = x % st, ym = y % st;
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < DVO_POINTS_PER_THREAD; k++) {
        bool ok = (k < nk) & (d[k] >= a.min_depth) & (d[k] <= a.max_depth) & (d[k] < __builtin_inff()) & (xm == 0) & (ym == 0);
        if (a.gate_sigma) ok = ok & (sg[k] <= a.max_sigma);
        if (a.age) ok = ok & (ag[k] >= a.min_age);
        if (a.counts) ok = ok & ((int)((c4 >> (8 * k)) & 0xffu) >= a.min_count);
        m |= (ok ? 1u : 0u) << k;
        xx++; xm++;
        if (xm == st) xm = 0;
        if (xx == a.w) { xx = 0; xm = 0; ym++; if (ym == st) ym = 0; }
    }
    return m;
}

__global__ void __launch_bounds__(256) k_points_count(PointsArgs a)
{
    const int seq = grid_seq();
    if (seq >= a.n_seq) return;
    if (!load_seq_entry(a.table, seq).on) return;   // uniform per workgroup
    const int n = a.w * a.h;
    const int i0 = ((int)blockIdx.x * 256 + (int)threadIdx.x) * DVO_POINTS_PER_THREAD;
    const int nk = i0 >= n ? 0 : (n - i0 < DVO_POINTS_PER_THREAD ? n - i0 : DVO_POINTS_PER_THREAD);
    float d[DVO_POINTS_PER_THREAD];
    int x, y;
    const uint32_t m = points_gates(a, (size_t)seq * n, i0, nk, d, x, y);
    uint32_t c = 0;   // the wave's points: four ballots (every lane of the wave is here)
#pragma unroll
    for (int k = 0; k < DVO_POINTS_PER_THREAD; k++) c += (uint32_t)__popcll(__ballot((m >> k) & 1u));
    __shared__ uint32_t wave_n[4];
    if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t t = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
        a.chunk_count[(size_t)seq * a.chunks + blockIdx.x] = t;
        if (t) atomicAdd(a.seq_total + seq, t);   // (an integer sum: the same total in any order)
    }
}

// offsets[s] = the totals of the sequences below s, offsets[n_seq] = the grand total: one workgroup, each thread a run of consecutive
// sequences, the 1 024 run sums scanned in LDS.
__global__ void __launch_bounds__(1024) k_points_scan(const uint32_t* __restrict__ seq_total, int n_seq, uint32_t* __restrict__ offsets,
                                                      uint32_t* __restrict__ offsets_out)
{
    __shared__ uint32_t part[1024];
    const int t = (int)threadIdx.x;
    const int per = (n_seq + 1023) / 1024;
    const int s0 = t * per < n_seq ? t * per : n_seq, s1 = s0 + per < n_seq ? s0 + per : n_seq;
    uint32_t sum = 0;
    for (int s = s0; s < s1; s++) sum += seq_total[s];
    part[t] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const uint32_t v = t >= o ? part[t - o] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t run = part[t] - sum;
    for (int s = s0; s < s1; s++) {
        offsets[s] = run;
        if (offsets_out) offsets_out[s] = run;
        run += seq_total[s];
    }
    if (t == 1023) {
        offsets[n_seq] = part[1023];
        if (offsets_out) offsets_out[n_seq] = part[1023];
    }
}

typedef float pt_f4 __attribute__((ext_vector_type(4)));

template <bool PCAM>
__device__ __forceinline__ void points_write(PointsArgs a)
{
    const int seq = grid_seq();
    if (seq >= a.n_seq) return;
    const PointsSeq e = load_seq_entry(a.table, seq);   // uniform per workgroup: scalar loads
    if (!e.on) return;
    const uint32_t* cc = a.chunk_count + (size_t)seq * a.chunks;
    const int chunk = (int)blockIdx.x;
    if (load_seq_entry(cc, chunk) == 0u) return;        // (the count pass found nothing here)
    uint32_t below = 0;   // this wave's share of the sequence's chunks below this one
    for (int c = (int)threadIdx.x; c < chunk; c += 256) below += cc[c];
    for (int o = 32; o > 0; o >>= 1) below += __shfl_xor(below, o);
    const int n = a.w * a.h;
    const int i0 = (chunk * 256 + (int)threadIdx.x) * DVO_POINTS_PER_THREAD;
    const int nk = i0 >= n ? 0 : (n - i0 < DVO_POINTS_PER_THREAD ? n - i0 : DVO_POINTS_PER_THREAD);
    const size_t base = (size_t)seq * n;
    float d[DVO_POINTS_PER_THREAD];
    int x, y;
    const uint32_t m = points_gates(a, base, i0, nk, d, x, y);
    uint32_t lanes_below = 0, wave_total = 0;   // points of the wave's lower lanes (mbcnt of each ballot), and of the wave
#pragma unroll
    for (int k = 0; k < DVO_POINTS_PER_THREAD; k++) {
        const unsigned long long b = __ballot((m >> k) & 1u);
        lanes_below = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, lanes_below));
        wave_total += (uint32_t)__popcll(b);
    }
    __shared__ uint32_t wave_below[4], wave_n[4];
    // the workgroup's points, staged in rank order: a lane's points are consecutive in the output, so storing them from the lane that
    // made them would put the 64 stores of a wave 64 bytes apart; out of LDS consecutive lanes store consecutive points
    __shared__ pt_f4 stage_p[DVO_POINTS_CHUNK];
    __shared__ uint32_t stage_src[DVO_POINTS_CHUNK];
    __shared__ float stage_sigma[DVO_POINTS_CHUNK];
    const int wv = (int)threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { wave_below[wv] = below; wave_n[wv] = wave_total; }
    __syncthreads();
    const uint32_t first = load_seq_entry(a.offsets, seq) + wave_below[0] + wave_below[1] + wave_below[2] + wave_below[3];
    const uint32_t total = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];   // (at most DVO_POINTS_CHUNK)
    if (first >= a.capacity) return;   // uniform: every point of the workgroup is at or past the capacity (counted, never written)
    uint32_t local = lanes_below;      // rank within the workgroup
    for (int v = 0; v < wv; v++) local += wave_n[v];
    Intr cam;
    if constexpr (PCAM) cam = load_seq_entry(a.seq_k, seq);
#pragma unroll
    for (int k = 0; k < DVO_POINTS_PER_THREAD; k++) {
        if ((m >> k) & 1u) {
            float X, Y, Z, Xw, Yw, Zw;
            back_project(map_intr<PCAM>(a, cam), (float)x, (float)y, d[k], X, Y, Z);
            transform(e.Wk, X, Y, Z, Xw, Yw, Zw);
            pt_f4 p;
            p.x = Xw; p.y = Yw; p.z = Zw; p.w = a.gray[base + i0 + k];
            stage_p[local] = p;
            stage_src[local] = (uint32_t)(i0 + k);
            if (a.sigma_out) stage_sigma[local] = a.sigma[base + i0 + k];
            local++;
        }
        x++;
        if (x == a.w) { x = 0; y++; }
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < total; j += 256) {
        const uint32_t r = first + j;
        if (r < a.capacity) {   // (a point at or past the capacity is counted, never written)
            reinterpret_cast<pt_f4*>(a.xyzg)[r] = stage_p[j];
            if (a.src) a.src[r] = stage_src[j];
            if (a.sigma_out) a.sigma_out[r] = stage_sigma[j];
        }
    }
}

__global__ void __launch_bounds__(256) k_points_write(PointsArgs a) { points_write<false>(a); }
__global__ void __launch_bounds__(256) k_points_write_cam(PointsArgs a) { points_write<true>(a); }

// ------------------------------------------------------------------------------------------------ launch wrappers
void launch_points_prep(const PointsPrepArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_points_prep, dim3(cdiv_u(a.n_seq, 64)), dim3(64), 0, s, a);
}

void launch_points(const PointsArgs& a0, uint32_t* offsets_out, hipStream_t s)
{
    PointsArgs a = a0;
    a.inv_w = 1.0f / (float)a.w;
    a.chunks = points_chunks(a.w, a.h);
    const dim3 grid = seq_grid((unsigned)a.chunks, (unsigned)a.n_seq);
    hipLaunchKernelGGL(k_points_count, grid, dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_points_scan, dim3(1), dim3(1024), 0, s, a.seq_total, a.n_seq, a.offsets, offsets_out);
    if (a.capacity == 0) return;   // the counting call
    if (a.seq_k) hipLaunchKernelGGL(k_points_write_cam, grid, dim3(256), 0, s, a);   // per-sequence intrinsics
    else hipLaunchKernelGGL(k_points_write, grid, dim3(256), 0, s, a);
}

void launch_kf_fuse_prep(const KfPrepArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_kf_fuse_prep, dim3(cdiv_u(a.n_seq, 64)), dim3(64), 0, s, a);
}

void launch_kf_carry_prep(const KfPrepArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_kf_carry_prep, dim3(cdiv_u(a.n_seq, 64)), dim3(64), 0, s, a);
}

// the pixel kernels of the fusion and of the carry: one lane per four top-level pixels; `cam` with per-sequence intrinsics
template <class Args>
static void launch_kf_pixels(void (*plain)(Args), void (*cam)(Args), const Args& a0, hipStream_t s)
{
    Args a = a0;
    const int T = a.levels - 1;
    a.inv_w = 1.0f / (float)a.w[T];
    const dim3 grid = seq_grid(cdiv_u(a.w[T] * a.h[T], 256 * DVO_KF_FUSE_PER_THREAD), (unsigned)a.n_seq);
    hipLaunchKernelGGL(a.seq_k ? cam : plain, grid, dim3(256), 0, s, a);
}
void launch_kf_fuse(const KfFuseArgs& a, hipStream_t s) { launch_kf_pixels(k_kf_fuse, k_kf_fuse_cam, a, s); }
void launch_kf_carry(const KfCarryArgs& a, hipStream_t s) { launch_kf_pixels(k_kf_carry, k_kf_carry_cam, a, s); }

void launch_kf_carry_commit(const KfCarryCommitArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_kf_carry_commit, seq_grid(cdiv_u(a.npix, 256 * 4), (unsigned)a.n_seq), dim3(256), 0, s, a);
}

void launch_mono_decide(MonoSeq* meta, const SeqState* state, int n_seq, int frame_id, float min_translation, int max_frames,
                        float* xi_world, float* T_world, int* is_key, const MonoRef* host_ref, hipStream_t s, int* need_list)
{
    MonoRef r{};
    if (host_ref) r = *host_ref;
    hipLaunchKernelGGL(k_mono_decide, dim3(cdiv_u(n_seq, 64)), dim3(64), 0, s, meta, state, n_seq, frame_id, min_translation, max_frames,
                       xi_world, T_world, is_key, r, need_list);
}

void launch_mono_commit(MonoSeq* meta, float* hist_xi, int n_seq, int R, int all, int frame_id, float* xi_world, float* T_world, int* is_key,
                        hipStream_t s)
{
    hipLaunchKernelGGL(k_mono_commit, dim3(cdiv_u(n_seq, 64)), dim3(64), 0, s, meta, hist_xi, n_seq, R, all, frame_id, xi_world, T_world, is_key);
}

void launch_age_table(const AgeTableArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_age_table, dim3(cdiv_u((unsigned)a.n_seq * (unsigned)a.R, 64)), dim3(64), 0, s, a);
}

void launch_promote(const PromoteArgs& a, hipStream_t s)
{
    int total = a.npix;
    bool vec = (a.npix % 4) == 0 && (reinterpret_cast<uintptr_t>(a.gray_top) % 16) == 0 && (reinterpret_cast<uintptr_t>(a.ring_gray) % 16) == 0;
    for (int g = 0; g < a.n_seg; g++) {
        total += a.count[g];
        vec = vec && (a.count[g] % 4) == 0 && (reinterpret_cast<uintptr_t>(a.src[g]) % 16) == 0 && (reinterpret_cast<uintptr_t>(a.dst[g]) % 16) == 0;
    }
    PromoteArgs b = a;
    const bool listed = !a.all && a.need_list != nullptr;
    b.n_slots = listed ? (a.n_seq < DVO_LIST_SLOTS ? a.n_seq : DVO_LIST_SLOTS) : 0;
    const unsigned gs = listed ? (unsigned)b.n_slots : (unsigned)a.n_seq;
    if (vec) hipLaunchKernelGGL(k_promote<4>, seq_grid(cdiv_u(total / 4, 256 * DVO_PROMOTE_PER_THREAD), gs), dim3(256), 0, s, b);
    else hipLaunchKernelGGL(k_promote<1>, seq_grid(cdiv_u(total, 256 * DVO_PROMOTE_PER_THREAD), gs), dim3(256), 0, s, b);
}

void launch_broadcast(const float* src, float* dst, int count, int n_seq, hipStream_t s)
{
    hipLaunchKernelGGL(k_broadcast, seq_grid(cdiv_u(count, 256), (unsigned)n_seq), dim3(256), 0, s, src, dst, count, n_seq);
}

void launch_propagate_batch(const PropArgs& a0, hipStream_t s)
{
    PropArgs a = a0;
    a.inv_w = 1.0f / (float)a.w;
    a.n_slots = a.need_list ? (a.n_seq < DVO_LIST_SLOTS ? a.n_seq : DVO_LIST_SLOTS) : 0;
    const dim3 grid = seq_grid(cdiv_u(a.w * a.h, 256 * DVO_PROP_PER_THREAD), a.need_list ? (unsigned)a.n_slots : (unsigned)a.n_seq);
    hipLaunchKernelGGL(k_propagate_init, grid, dim3(256), 0, s, a);
    if (a.seq_k) hipLaunchKernelGGL(k_propagate_owner_cam, grid, dim3(256), 0, s, a);   // per-sequence intrinsics
    else hipLaunchKernelGGL(k_propagate_owner, grid, dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_propagate_pull, grid, dim3(256), 0, s, a);
}

void launch_propagate(const float* ref_depth, const float* ref_sigma, const float* ref_age, int w, int h, const Intr& k,
                      const Pose& pose, float tz, int* owner, float* depth, float* sigma, float* age, hipStream_t s)
{
    PropArgs a{};
    a.ref_depth = ref_depth; a.ref_sigma = ref_sigma; a.ref_age = ref_age;
    a.depth = depth; a.sigma = sigma; a.age = age; a.owner = owner;
    a.w = w; a.h = h; a.n_seq = 1; a.k = k; a.pose = pose; a.tz = tz;
    launch_propagate_batch(a, s);
}

void launch_regularize_batch(const float* depth, const float* sigma, int w, int h, int n_seq, float* out, hipStream_t s)
{
    hipLaunchKernelGGL(k_regularize, seq_grid(cdiv_u(w * h, 256), (unsigned)n_seq), dim3(256), 0, s, depth, sigma, w, h, n_seq, 1.0f / (float)w, out);
}

void launch_regularize_redecimate(const RegDecArgs& a0, hipStream_t s)
{
    RegDecArgs a = a0;
    const int T = a.levels - 1;
    a.inv_w = 1.0f / (float)a.w[T];
    hipLaunchKernelGGL(k_regularize_redecimate, seq_grid(cdiv_u(a.w[T] * a.h[T], 256), (unsigned)a.n_seq), dim3(256), 0, s, a);
}

void launch_mono_decide_plan(const MonoPlanArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_mono_decide_plan, dim3(cdiv_u(a.n_seq, 64)), dim3(64), 0, s, a);
}

void launch_mono_commit_plan(const MonoPlanArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_mono_commit_plan, dim3(cdiv_u(a.n_seq, 64)), dim3(64), 0, s, a);
}

void launch_kf_decide(const MonoPlanArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_kf_decide, dim3(cdiv_u(a.n_seq, 64)), dim3(64), 0, s, a);
}

void launch_mono_seed(const PoseSeedArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_mono_seed, dim3(cdiv_u(a.n_seq, 64)), dim3(64), 0, s, a);
}

void launch_regularize_redecimate_plan(const RegDecArgs& a0, const MonoStartArgs& p, hipStream_t s)
{
    RegDecArgs a = a0;
    const int T = a.levels - 1;
    a.inv_w = 1.0f / (float)a.w[T];
    hipLaunchKernelGGL(k_regularize_redecimate_plan, seq_grid(cdiv_u(a.w[T] * a.h[T], 256), (unsigned)a.n_seq), dim3(256), 0, s, a, p);
}

void launch_regularize(const float* depth, const float* sigma, int w, int h, float* out, hipStream_t s)
{
    launch_regularize_batch(depth, sigma, w, h, 1, out, s);
}

void launch_depth_update(const UpdateArgs& a0, hipStream_t s)
{
    UpdateArgs a = a0;
    const int ww = a.crop ? ((a.w - 1 < 144 ? a.w - 1 : 144) - 16 + 1) : a.w, wh = a.crop ? ((a.h - 1 < 108 ? a.h - 1 : 108) - 12 + 1) : a.h;
    if (ww <= 0 || wh <= 0) return;
    a.inv_ww = 1.0f / (float)ww;
    a.k_sparse = k9_sparse(a.K9);
    const dim3 grid = seq_grid(cdiv_u(ww * wh, 256), (unsigned)a.n_seq);
    if (a.seq_k) hipLaunchKernelGGL(k_depth_update_cam, grid, dim3(256), 0, s, a);   // per-sequence intrinsics (a.seq_K9 set too)
    else hipLaunchKernelGGL(k_depth_update, grid, dim3(256), 0, s, a);
}

}  // namespace dvo
