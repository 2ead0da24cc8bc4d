// dvo_kernels.hip -- hand-written CDNA4 (gfx950) kernels of the direct-VO hot path.
//
// wave64, 256-thread workgroups, no MFMA (image warping bound by the vector ALUs and the L1 gather path).
// Reductions are fixed-order (DPP row_shr / row_bcast inside a wave, LDS across the 4 waves, double
// across workgroups) so every run is bit-reproducible.  Built with -ffp-contract=off: only the fmaf()
// calls written in dvo_math.h fuse.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <type_traits>

#include "dvo_kernels.h"

namespace dvo {

// ------------------------------------------------------------------------------------------------
// helpers
// ------------------------------------------------------------------------------------------------
// XCD-aware bijective remap of the linear workgroup id: workgroups b and b+8 share an XCD (round-robin
// dispatch), so give each XCD one contiguous range of tiles -> neighbouring tiles of an image (which share
// gather rows of ref_gray) hit the same 4 MiB L2.  Speed only, never correctness.
__device__ __forceinline__ unsigned xcd_remap(unsigned bid, unsigned nwg)
{
    const unsigned xcd = bid & 7u, q = nwg >> 3, r = nwg & 7u;
    const unsigned base = (xcd < r) ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q;
    return base + (bid >> 3);
}

// wave64 sum, result valid in lane 63.  Classic GCN scan: row_shr 1,2,4,8 inside each row of 16 lanes,
// then row_bcast:15 into rows 1,3 and row_bcast:31 into rows 2,3.  Fixed order => deterministic.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_step(float v)
{
    const int moved = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xf, false);
    return v + __int_as_float(moved);
}

__device__ __forceinline__ float wave_sum_to_lane63(float v)
{
    v = dpp_step<0x111, 0xf>(v);  // row_shr:1
    v = dpp_step<0x112, 0xf>(v);  // row_shr:2
    v = dpp_step<0x114, 0xf>(v);  // row_shr:4
    v = dpp_step<0x118, 0xf>(v);  // row_shr:8
    v = dpp_step<0x142, 0xa>(v);  // row_bcast:15 -> rows 1 and 3
    v = dpp_step<0x143, 0xc>(v);  // row_bcast:31 -> rows 2 and 3
    return v;
}

// ------------------------------------------------------------------------------------------------
// Packed wave64 reduction of 29 per-lane accumulators (fixed order, deterministic).
// A plain butterfly spends 6 DPP adds per value (174 VALU per wave) although half of the lanes carry useful data
// after every step.  Here every step also PACKS two registers into one, so the work halves each time (68 VALU):
//   32-lane step: v_permlane32_swap (gfx950) of a register pair + 1 add  -> low half = sum of A, high half = sum of B
//   16-lane step: v_permlane16_swap of a pair + 1 add                    -> one value per 16-lane row
//    8-lane step: row_shl:8 / row_shr:8 DPP adds of a pair + bank-masked merge -> one value per 8 lanes
//    4-lane step: row_shl:4 / row_shr:4, same                            -> one value per quad (2 registers left)
//    quad steps : quad_perm adds                                         -> every lane of a quad holds its value's total
// Lane L of output register q then holds value  16 q + {0,8,4,12}[(L>>2)&3] + {0,2,1,3}[L>>4].
// ------------------------------------------------------------------------------------------------
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float swap32_add(float a, float b)
{
    const u32x2 r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r.x) + __uint_as_float(r.y);
}
__device__ __forceinline__ float swap16_add(float a, float b)
{
    const u32x2 r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r.x) + __uint_as_float(r.y);
}
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
// lanes selected by BANK_MASK (4-lane banks inside each 16-lane row) take `hi`, the others keep `lo`
template <int BANK_MASK>
__device__ __forceinline__ float bank_merge(float lo, float hi)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(lo), __float_as_int(hi), 0xE4 /*quad_perm identity*/, 0xf, BANK_MASK, false));
}

__device__ __forceinline__ int packed_slot_index(int lane, int q)
{
    const int quad = (lane >> 2) & 3, row = lane >> 4;
    const int qm = (quad == 0) ? 0 : (quad == 1) ? 8 : (quad == 2) ? 4 : 12;
    const int rm = (row == 0) ? 0 : (row == 1) ? 2 : (row == 2) ? 1 : 3;
    return 16 * q + qm + rm;
}

// v[0..28] in, out0/out1 as described above
__device__ __forceinline__ void wave_reduce29_packed(const float* v, float& out0, float& out1)
{
    float A[15];
#pragma unroll
    for (int j = 0; j < 14; j++) A[j] = swap32_add(v[2 * j], v[2 * j + 1]);
    A[14] = swap32_add(v[28], 0.0f);
    float B[8];
#pragma unroll
    for (int m = 0; m < 7; m++) B[m] = swap16_add(A[2 * m], A[2 * m + 1]);
    B[7] = swap16_add(A[14], 0.0f);
    float Cc[4];
#pragma unroll
    for (int n = 0; n < 4; n++) {
        const float lo = B[2 * n] + dpp_mov<0x108>(B[2 * n]);          // row_shl:8 -> lanes 0-7 of each row
        const float hi = B[2 * n + 1] + dpp_mov<0x118>(B[2 * n + 1]);  // row_shr:8 -> lanes 8-15
        Cc[n] = bank_merge<0xC>(lo, hi);
    }
    float D[2];
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const float lo = Cc[2 * q] + dpp_mov<0x104>(Cc[2 * q]);          // row_shl:4 -> lanes 0-3, 8-11
        const float hi = Cc[2 * q + 1] + dpp_mov<0x114>(Cc[2 * q + 1]);  // row_shr:4 -> lanes 4-7, 12-15
        D[q] = bank_merge<0xA>(lo, hi);
    }
#pragma unroll
    for (int q = 0; q < 2; q++) {
        D[q] = D[q] + dpp_mov<0xB1>(D[q]);  // quad_perm [1,0,3,2]
        D[q] = D[q] + dpp_mov<0x4E>(D[q]);  // quad_perm [2,3,0,1]
    }
    out0 = D[0];
    out1 = D[1];
}

__device__ __forceinline__ void split_index(int i, int w, float inv_w, int& x, int& y)
{  // i < 2^24: y = i / w without an integer divide; the +-1 fix-up is branch free
    y = (int)((float)i * inv_w);
    x = i - y * w;
    const int lo = x < 0 ? 1 : 0, hi = x >= w ? 1 : 0;
    y += hi - lo;
    x += (lo - hi) * w;
}

// ------------------------------------------------------------------------------------------------
// Building blocks of the pyramid-build kernels: what the kernels of the family below share, stated once.  A
// kernel whose instruction stream is pinned (tests/golden/isa_*.json) keeps written out each piece under whose helper the stream
// moves, and says so in one line: all of k_pyramid and k_pyramid_raw4, the walk of k_pyramid_remap.
// ------------------------------------------------------------------------------------------------
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));

// The 8-bit luma of pixel `off` of a raw frame: the byte itself, or k_ingest's fixed-point weights of R, G and B (A is not read)
__device__ __forceinline__ unsigned raw_luma8(const PyramidArgs& a, size_t off)
{
    unsigned g8;
    if (a.raw_channels == 1) {
        g8 = __builtin_nontemporal_load(a.raw_rgb + off);
    } else {
        const uint8_t* p = a.raw_rgb + off * (size_t)a.raw_channels;
        g8 = ((unsigned)p[0] * 4899u + (unsigned)p[1] * 9617u + (unsigned)p[2] * 1868u + 8192u) >> 14;
    }
    return g8;
}

// k_ingest's conversion of one raw pixel with depth (the same float operations): luma g8 and depth word d to gray, depth and
// sigma; a pixel without a depth reading has no gray either (raw_invalidate_gray, transform.cpp:60-76).  The argument block by
// value: through a reference the loads of its five constants repeat per pixel (k_pyramid_raw4_rest<2>: +2 VGPRs).
struct RawPixel { float gray, depth, sigma; };
__device__ __forceinline__ RawPixel raw_convert(const PyramidArgs a, unsigned g8, unsigned d)
{
    RawPixel p;
    p.gray = (float)g8 * a.raw_gray_scale;
    if (a.raw_invalidate_gray && d == 0) p.gray = kInvalid;
    p.depth = (float)d * a.raw_depth_scale;
    p.sigma = d > 0 ? a.raw_sigma_valid : a.raw_sigma_invalid;
    return p;
}

// The packed words of the 4 << SHIFT consecutive pixels of one row that a thread of a four-pixel kernel reads from 1-channel u8
// gray and u16 depth, 16 bytes per load (8 for the two gray words of SHIFT 1); kept pixel k of the thread is pixel k << SHIFT.
template <int SHIFT>
struct RawWords {
    static constexpr int GW = 1 << SHIFT;   // 32-bit words of gray bytes
    unsigned g[GW], d[2 * GW];
    __device__ __forceinline__ void load_gray(const PyramidArgs& a, size_t off)
    {
        if constexpr (SHIFT == 1) {
            const u32x2 v = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(a.raw_rgb + off));
            g[0] = v.x; g[1] = v.y;
        } else {
            const u32x4* gp = reinterpret_cast<const u32x4*>(a.raw_rgb + off);
#pragma unroll
            for (int q = 0; q < GW / 4; q++) {
                const u32x4 v = __builtin_nontemporal_load(gp + q);
                g[4 * q] = v.x; g[4 * q + 1] = v.y; g[4 * q + 2] = v.z; g[4 * q + 3] = v.w;
            }
        }
    }
    __device__ __forceinline__ void load_depth(const PyramidArgs& a, size_t off)
    {
        const u32x4* dp = reinterpret_cast<const u32x4*>(a.raw_depth + off);
#pragma unroll
        for (int q = 0; q < GW / 2; q++) {
            const u32x4 v = __builtin_nontemporal_load(dp + q);
            d[4 * q] = v.x; d[4 * q + 1] = v.y; d[4 * q + 2] = v.z; d[4 * q + 3] = v.w;
        }
    }
    __device__ __forceinline__ unsigned gray8(int k) const { const int si = k << SHIFT; return (g[si >> 2] >> ((si & 3) * 8)) & 0xffu; }
    __device__ __forceinline__ unsigned depth16(int k) const { const int si = k << SHIFT; return (d[si >> 1] >> ((si & 1) * 16)) & 0xffffu; }
};

// The level rule: level t below a thread's own level keeps the pixels whose coordinates are multiples of 2^t.  The thread owns
// pixels (x0 .. x0 + PPT - 1, y) of level n - 1; f(l, o, k) runs for every level l = n - 1 - t, T0 <= t < n, that keeps its pixel
// k, with o the offset of that pixel in level l of sequence seq.  T0 = 1: the thread stores its own level itself (16-byte stores).
template <int PPT, int T0, class F>
__device__ __forceinline__ void walk_levels(const PyramidArgs& a, int n, int seq, int x0, int y, F&& f)
{
    for (int t = T0; t < n; t++) {
        const int msk = (1 << t) - 1;
        if constexpr (PPT == 1) {
            if ((x0 & msk) | (y & msk)) break;
            const int l = n - 1 - t, lx = x0 >> t, ly = y >> t;
            if (lx >= a.w[l] || ly >= a.h[l]) continue;   // (a level of odd size has fewer pixels than its parent's even coordinates)
            f(l, (size_t)seq * a.w[l] * a.h[l] + (size_t)ly * a.w[l] + lx, 0);
        } else {
            if (y & msk) break;
            const int l = n - 1 - t, ly = y >> t;
            if (ly >= a.h[l]) continue;
#pragma unroll
            for (int k = 0; k < PPT; k++) {
                const int x = x0 + k;
                if (x & msk) continue;
                const int lx = x >> t;
                if (lx >= a.w[l]) continue;
                f(l, (size_t)seq * a.w[l] * a.h[l] + (size_t)ly * a.w[l] + lx, k);
            }
        }
    }
}

// The DVO_SEQ_SKIP rule of a planned build (PyramidArgs::seq_action).  The sequence comes from blockIdx.y/z, so the answer is
// uniform per workgroup.  A build with a reference set copies forward: the thread takes the reference's top-level values in
// place of the ones it would build and stores them as a build does (lower levels through pass_valid, which is what the
// reference's build stored there; wgt copied level by level).  A mono build with a remap has no reference set and writes nothing.
__device__ __forceinline__ bool seq_skips(const PyramidArgs& a, int seq) { return a.seq_action[seq] == DVO_SEQ_SKIP; }

// ------------------------------------------------------------------------------------------------
// k_pyramid: System::Frame pyramid (frame.hpp:91-117, frame.cpp:16-37) = nearest-neighbour decimation
// (Convert::cullImage, convert.cpp:7-20) of up to three maps, all levels in ONE launch.
// One thread per TOP-level pixel reads src(x<<culls, y<<culls) once and writes every level it lands on
// (level t shifts below the top keep pixels whose coordinates are multiples of 2^t).
// ------------------------------------------------------------------------------------------------
// PLAN (Batch plan, PyramidArgs::seq_action): the workgroups of a DVO_SEQ_SKIP sequence copy the reference set's values forward instead
// (the sequence comes from blockIdx.y/z: the branch is uniform per workgroup).  PLAN = false is the plain build.
template <bool PLAN>
__global__ void __launch_bounds__(256) k_pyramid(PyramidArgs a)
{
    const int tw = a.w[a.levels - 1], th = a.h[a.levels - 1];
    const int seq = (int)(blockIdx.z * DVO_GRID_SEQ_Y + blockIdx.y);   // seq_grid() (dvo_kernels.h): no division, no 65535 limit
    const int i = (int)blockIdx.x * 256 + threadIdx.x;
    if (i >= tw * th || seq >= a.n_seq) return;
    int x, y;
    split_index(i, tw, a.inv_tw, x, y);
    if constexpr (PLAN) {
        if (a.seq_action[seq] == DVO_SEQ_SKIP) {   // copy_forward<1> written out: under the helper the pinned stream moves
            const int T = a.levels - 1;
            const size_t ot = (size_t)seq * tw * th + (size_t)y * tw + x;
            bool have[3];
            have[0] = true;
            have[1] = have[2] = a.raw_rgb != nullptr ? a.raw_depth != nullptr : false;
            if (a.raw_rgb == nullptr)
                for (int m = 0; m < 3; m++) have[m] = a.src[m] != nullptr;
            const bool prep = a.wgt[0] != nullptr && have[1] && have[2];
            float top[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int m = 0; m < 3; m++)
                if (have[m] && a.dst[m][T] != nullptr) top[m] = __builtin_nontemporal_load(a.ref[m][T] + ot);
            for (int t = 0; t < a.levels; t++) {
                const int msk = (1 << t) - 1;
                if ((x & msk) | (y & msk)) break;
                const int l = a.levels - 1 - t, lx = x >> t, ly = y >> t;
                if (lx >= a.w[l] || ly >= a.h[l]) continue;
                const size_t o = (size_t)seq * a.w[l] * a.h[l] + (size_t)ly * a.w[l] + lx;
#pragma unroll
                for (int m = 0; m < 3; m++)
                    if (have[m] && a.dst[m][l] != nullptr) __builtin_nontemporal_store(t == 0 ? top[m] : pass_valid(top[m]), a.dst[m][l] + o);
                if (prep) __builtin_nontemporal_store(__builtin_nontemporal_load(a.ref_wgt[l] + o), a.wgt[l] + o);
            }
            return;
        }
    }
    const size_t src_off = (size_t)seq * a.src_w * a.src_img_rows + (size_t)(y << a.src_row_shift) * a.src_w + (x << a.culls);
    float raw[3] = {0.0f, 0.0f, 0.0f};
    bool have[3];
    if (a.raw_rgb != nullptr) {  // raw sensor frame: convert exactly as k_ingest does (same float operations), only the kept pixels
        // raw_luma8 and raw_convert written out: under either helper the pinned stream moves
        unsigned g8;
        if (a.raw_channels == 1) {
            g8 = __builtin_nontemporal_load(a.raw_rgb + src_off);
        } else {
            const uint8_t* p = a.raw_rgb + src_off * (size_t)a.raw_channels;
            g8 = ((unsigned)p[0] * 4899u + (unsigned)p[1] * 9617u + (unsigned)p[2] * 1868u + 8192u) >> 14;
        }
        raw[0] = (float)g8 * a.raw_gray_scale;
        have[0] = true; have[1] = have[2] = a.raw_depth != nullptr;
        if (a.raw_depth != nullptr) {
            const unsigned d = __builtin_nontemporal_load(a.raw_depth + src_off);
            raw[1] = (float)d * a.raw_depth_scale;
            raw[2] = d > 0 ? a.raw_sigma_valid : a.raw_sigma_invalid;
            if (a.raw_invalidate_gray && d == 0) raw[0] = kInvalid;
        }
    } else {
#pragma unroll
        for (int m = 0; m < 3; m++) {
            have[m] = a.src[m] != nullptr;
            if (have[m]) raw[m] = __builtin_nontemporal_load(a.src[m] + src_off);  // read once: streamed past the caches; the three loads are in flight together
        }
    }
    // the reference-frame constants of k_prep_ref, written while depth and sigma are in registers (needs both maps)
    const bool prep = a.wgt[0] != nullptr && have[1] && have[2];
    for (int t = 0; t < a.levels; t++) {   // walk_levels<1, 0> written out: under the helper the pinned stream moves
        const int msk = (1 << t) - 1;
        if ((x & msk) | (y & msk)) break;
        const int l = a.levels - 1 - t, lx = x >> t, ly = y >> t;
        if (lx >= a.w[l] || ly >= a.h[l]) continue;
        const size_t o = (size_t)seq * a.w[l] * a.h[l] + (size_t)ly * a.w[l] + lx;
        float val[3];
#pragma unroll
        for (int m = 0; m < 3; m++) {
            // top level: cullImage(src, culls); culls == 0 aliases the input (convert.cpp:9-10), no pass_valid
            val[m] = (t == 0 && a.culls == 0) ? raw[m] : pass_valid(raw[m]);
            if (have[m] && a.dst[m][l] != nullptr) __builtin_nontemporal_store(val[m], a.dst[m][l] + o);  // (a map may be consumed without being kept; next read: a whole tracking step later)
        }
        if (prep) __builtin_nontemporal_store(gn_weight(a.step[l], a.sigma_min, a.sigma_max, val[2]), a.wgt[l] + o);
    }
}

// k_pyramid_remap: k_pyramid of MONO frames (gray only) with the lens undistortion fused in (dvo_batch_set_distortion,
// dvo_vo_set_distortion).  Under nearest-neighbour remapping, kept pixel (x << culls, y << culls) of the undistorted frame is ONE
// pixel of the distorted input: the thread reads its index from the sequence's camera table (k_undistort_map; -1 = outside the
// image = k_undistort's INVALID border), gathers that one u8 (k_pyramid's raw conversion) or float, and writes every level as
// k_pyramid does.  The same operations as k_undistort followed by k_pyramid: bit-identical, and no undistorted frame is stored.
// The table is read with plain loads (it is shared by every sequence of the camera and stays in L2), the frame and the levels
// with k_pyramid's nontemporal accesses.  The input holds whole frames (src_img_rows = src_h): the gather reads any row.
// remap_gather_gray is that gather, shared with k_pyramid_remap_plan.
__device__ __forceinline__ float remap_gather_gray(const PyramidArgs& a, int seq, int tw, int th, int x, int y)
{
    const int cam = load_seq_entry(a.remap_cam, seq);   // (uniform per workgroup: one scalar load)
    const int si = a.remap[(size_t)cam * tw * th + (size_t)y * tw + x];
    float raw = kInvalid;
    if (si >= 0) {
        const size_t src_off = (size_t)seq * a.src_w * a.src_h + (size_t)si;
        if (a.raw_rgb != nullptr) raw = (float)raw_luma8(a, src_off) * a.raw_gray_scale;
        else raw = __builtin_nontemporal_load(a.src[0] + src_off);
    }
    return raw;
}

__global__ void __launch_bounds__(256) k_pyramid_remap(PyramidArgs a)
{
    const int tw = a.w[a.levels - 1], th = a.h[a.levels - 1];
    const int seq = (int)(blockIdx.z * DVO_GRID_SEQ_Y + blockIdx.y);
    const int i = (int)blockIdx.x * 256 + threadIdx.x;
    if (i >= tw * th || seq >= a.n_seq) return;
    int x, y;
    split_index(i, tw, a.inv_tw, x, y);
    const float raw = remap_gather_gray(a, seq, tw, th, x, y);
    for (int t = 0; t < a.levels; t++) {   // walk_levels<1, 0> written out: under the helper the pinned stream moves
        const int msk = (1 << t) - 1;
        if ((x & msk) | (y & msk)) break;
        const int l = a.levels - 1 - t, lx = x >> t, ly = y >> t;
        if (lx >= a.w[l] || ly >= a.h[l]) continue;
        const size_t o = (size_t)seq * a.w[l] * a.h[l] + (size_t)ly * a.w[l] + lx;
        __builtin_nontemporal_store((t == 0 && a.culls == 0) ? raw : pass_valid(raw), a.dst[0][l] + o);
    }
}

// k_pyramid_remap_plan: k_pyramid_remap in a planned mono call (dvo_batch_set_mono_actions): the workgroups of a DVO_SEQ_SKIP
// sequence return at once.  Its slot of the input is never read and its slice of the frame set is left as it was: nothing
// downstream reads the frame of a sequence that does not track or start.  The same gather, then the walk through the helper; a
// kernel of its own because k_pyramid_remap's stream is pinned and moves under any shared body (by reference or by value).
__global__ void __launch_bounds__(256) k_pyramid_remap_plan(PyramidArgs a)
{
    const int tw = a.w[a.levels - 1], th = a.h[a.levels - 1];
    const int seq = (int)(blockIdx.z * DVO_GRID_SEQ_Y + blockIdx.y);
    const int i = (int)blockIdx.x * 256 + threadIdx.x;
    if (i >= tw * th || seq >= a.n_seq) return;
    if (seq_skips(a, seq)) return;
    int x, y;
    split_index(i, tw, a.inv_tw, x, y);
    const float raw = remap_gather_gray(a, seq, tw, th, x, y);
    walk_levels<1, 0>(a, a.levels, seq, x, y, [&](int l, size_t o, int) {
        __builtin_nontemporal_store((l == a.levels - 1 && a.culls == 0) ? raw : pass_valid(raw), a.dst[0][l] + o);
    });
}

// k_pyramid_raw4: the raw-sensor form of k_pyramid for 1-channel u8 gray (+ u16 depth) with CULLS = 1 or 2, four kept pixels
// per thread.  The scalar form spends one byte / short load per lane (a full vector-memory instruction for 1-2 useful bytes and
// half-empty sectors); here a thread owns 4 consecutive top-level pixels = 4 << CULLS source pixels of one row, fetched by one or
// two dwordx2/x4 loads, and writes its four top-level values per map as one dwordx4 store.  Same conversions, same float
// operations as k_ingest + k_pyramid: bit-identical (tests/test_frontend_and_eval.py).
// RawWords, raw_convert, walk_levels<4, 1> and the copy-forward written out: under each helper the pinned stream moves (DESIGN.md
// §32).  k_pyramid_raw4_rest below is this kernel's plain build in terms of them.
template <int CULLS, bool PLAN>
__global__ void __launch_bounds__(256) k_pyramid_raw4(PyramidArgs a)
{
    const int tw = a.w[a.levels - 1], th = a.h[a.levels - 1], gw = tw >> 2;
    const int seq = (int)(blockIdx.z * DVO_GRID_SEQ_Y + blockIdx.y);
    const int gi = (int)blockIdx.x * 256 + threadIdx.x;
    if (gi >= gw * th || seq >= a.n_seq) return;
    int y, xg;
    split_index(gi, gw, a.inv_tw * 4.0f, xg, y);   // (4 / tw = 1 / gw up to an ulp: split_index corrects +-1)
    const int x0 = xg << 2;
    if constexpr (PLAN) {
        if (a.seq_action[seq] == DVO_SEQ_SKIP) {   // copy-forward (see k_pyramid): the four top-level values per map, one 16-byte load each
            const bool dep = a.raw_depth != nullptr, prep = a.wgt[0] != nullptr && dep;
            const int T = a.levels - 1;
            const size_t ot = (size_t)seq * tw * th + (size_t)y * tw + x0;
            f4 top[3];
#pragma unroll
            for (int m = 0; m < 3; m++) {
                top[m] = f4{0.0f, 0.0f, 0.0f, 0.0f};
                if ((m == 0 || dep) && a.dst[m][T] != nullptr) {
                    top[m] = __builtin_nontemporal_load(reinterpret_cast<const f4*>(a.ref[m][T] + ot));
                    __builtin_nontemporal_store(top[m], reinterpret_cast<f4*>(a.dst[m][T] + ot));
                }
            }
            if (prep) __builtin_nontemporal_store(__builtin_nontemporal_load(reinterpret_cast<const f4*>(a.ref_wgt[T] + ot)),
                                                  reinterpret_cast<f4*>(a.wgt[T] + ot));
            for (int t = 1; t < a.levels; t++) {
                const int msk = (1 << t) - 1;
                if (y & msk) break;
                const int l = a.levels - 1 - t, ly = y >> t;
                if (ly >= a.h[l]) continue;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int x = x0 + k;
                    if (x & msk) continue;
                    const int lx = x >> t;
                    if (lx >= a.w[l]) continue;
                    const size_t o = (size_t)seq * a.w[l] * a.h[l] + (size_t)ly * a.w[l] + lx;
#pragma unroll
                    for (int m = 0; m < 3; m++)
                        if ((m == 0 || dep) && a.dst[m][l] != nullptr) __builtin_nontemporal_store(pass_valid(top[m][k]), a.dst[m][l] + o);
                    if (prep) __builtin_nontemporal_store(__builtin_nontemporal_load(a.ref_wgt[l] + o), a.wgt[l] + o);
                }
            }
            return;
        }
    }
    const size_t src_off = (size_t)seq * a.src_w * a.src_img_rows + (size_t)(y << a.src_row_shift) * a.src_w + ((size_t)x0 << CULLS);
    constexpr int GW = 1 << CULLS;       // 32-bit words of gray bytes this thread reads (2 or 4)
    unsigned gwords[GW], dwords[2 * GW];
    const bool dep = a.raw_depth != nullptr;
    {
        const unsigned* gp = reinterpret_cast<const unsigned*>(a.raw_rgb + src_off);
        if constexpr (CULLS == 1) { const u32x2 v = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(gp)); gwords[0] = v.x; gwords[1] = v.y; }
        else { const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(gp)); gwords[0] = v.x; gwords[1] = v.y; gwords[2] = v.z; gwords[3] = v.w; }
        if (dep) {
            const u32x4* dp = reinterpret_cast<const u32x4*>(a.raw_depth + src_off);
#pragma unroll
            for (int q = 0; q < GW / 2; q++) {
                const u32x4 v = __builtin_nontemporal_load(dp + q);
                dwords[4 * q] = v.x; dwords[4 * q + 1] = v.y; dwords[4 * q + 2] = v.z; dwords[4 * q + 3] = v.w;
            }
        }
    }
    float raw[4][3];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int si = k << CULLS;                                            // source pixel of kept pixel k
        const unsigned g8 = (gwords[si >> 2] >> ((si & 3) * 8)) & 0xffu;
        raw[k][0] = (float)g8 * a.raw_gray_scale;
        raw[k][1] = 0.0f; raw[k][2] = 0.0f;
        if (dep) {
            const unsigned d = (dwords[si >> 1] >> ((si & 1) * 16)) & 0xffffu;
            raw[k][1] = (float)d * a.raw_depth_scale;
            raw[k][2] = d > 0 ? a.raw_sigma_valid : a.raw_sigma_invalid;
            if (a.raw_invalidate_gray && d == 0) raw[k][0] = kInvalid;
        }
    }
    const bool prep = a.wgt[0] != nullptr && dep;
    // top level (t = 0): cullImage(src, CULLS >= 1) -> pass_valid; four values per map, one 16-byte store
    {
        const int l = a.levels - 1;
        const size_t o = (size_t)seq * tw * th + (size_t)y * tw + x0;
        f4 v[3], wgv;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float g = pass_valid(raw[k][0]), d = pass_valid(raw[k][1]), sg = pass_valid(raw[k][2]);
            v[0][k] = g; v[1][k] = d; v[2][k] = sg;
            wgv[k] = gn_weight(a.step[l], a.sigma_min, a.sigma_max, sg);
        }
        __builtin_nontemporal_store(v[0], reinterpret_cast<f4*>(a.dst[0][l] + o));
        if (dep && a.dst[1][l]) __builtin_nontemporal_store(v[1], reinterpret_cast<f4*>(a.dst[1][l] + o));
        if (dep && a.dst[2][l]) __builtin_nontemporal_store(v[2], reinterpret_cast<f4*>(a.dst[2][l] + o));
        if (prep) __builtin_nontemporal_store(wgv, reinterpret_cast<f4*>(a.wgt[l] + o));
    }
    for (int t = 1; t < a.levels; t++) {   // lower levels: pixels whose coordinates are multiples of 2^t
        const int msk = (1 << t) - 1;
        if (y & msk) break;
        const int l = a.levels - 1 - t, ly = y >> t;
        if (ly >= a.h[l]) continue;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int x = x0 + k;
            if (x & msk) continue;
            const int lx = x >> t;
            if (lx >= a.w[l]) continue;
            const size_t o = (size_t)seq * a.w[l] * a.h[l] + (size_t)ly * a.w[l] + lx;
            const float g = pass_valid(raw[k][0]), d = pass_valid(raw[k][1]), sg = pass_valid(raw[k][2]);
            __builtin_nontemporal_store(g, a.dst[0][l] + o);
            if (dep && a.dst[1][l]) __builtin_nontemporal_store(d, a.dst[1][l] + o);
            if (dep && a.dst[2][l]) __builtin_nontemporal_store(sg, a.dst[2][l] + o);
            if (prep) __builtin_nontemporal_store(gn_weight(a.step[l], a.sigma_min, a.sigma_max, sg), a.wgt[l] + o);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Photometric calibration fused into the mono ingest (dvo_batch_set_photometric, dvo_vo_set_photometric).  The
// kernels below run only on a handle with a calibration and take PhotoArgs beside PyramidArgs; every kernel above is untouched.
// For a kept pixel with byte (or fixed-point luma) g8:  gray = response[cal][g8] * gain[pair][y][x], one float multiply, where
// gain = 1 / vignette at the pixel's source was divided once by k_photometric_map; gain < 0 (kPhotoMasked) gives DVO_INVALID.
// Then the levels are written exactly as the plain kernels write them (pass_valid at the top level: culls >= 1 on this path).
//
// The response row of the workgroup's sequence (1 KB, uniform per workgroup) is staged in LDS by the 256 threads, one entry each,
// before any thread can leave: only the uniform seq >= n_seq exit comes first.  RESP_LDS = false is the other form, plain loads
// from the cached table (DVO_PHOTO_RESPONSE=global: A/B runs, tools/bench_photometric.py).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float photo_gray(float response, float gain) { return gain < 0.0f ? kInvalid : response * gain; }

// k_pyramid_raw4_photo: k_pyramid_raw4 of mono frames (1-channel u8, gray only, CULLS = 2) with the calibration.  Per thread one
// 16-byte load of source bytes, one 16-byte load of its four gains (plain: the table is shared by every sequence of the pair and
// stays in L2), four response lookups, one 16-byte top-level store and k_pyramid_raw4's lower-level stores.
template <int CULLS, bool PLAN, bool RESP_LDS>
__global__ void __launch_bounds__(256) k_pyramid_raw4_photo(PyramidArgs a, PhotoArgs p)
{
    static_assert(CULLS == 2, "the mono geometry: Frame(gray, K, 3, 2)");
    __shared__ float lut[256];
    const int tw = a.w[a.levels - 1], th = a.h[a.levels - 1], gw = tw >> 2;
    const int seq = (int)(blockIdx.z * DVO_GRID_SEQ_Y + blockIdx.y);
    if (seq >= a.n_seq) return;   // (uniform per workgroup)
    const float* resp = p.response + (size_t)load_seq_entry(p.seq_cal, seq) * 256;
    if constexpr (RESP_LDS) {
        lut[threadIdx.x] = resp[threadIdx.x];
        __syncthreads();
    }
    const int gi = (int)blockIdx.x * 256 + threadIdx.x;
    if (gi >= gw * th) return;
    int y, xg;
    split_index(gi, gw, a.inv_tw * 4.0f, xg, y);
    const int x0 = xg << 2;
    const size_t ot = (size_t)seq * tw * th + (size_t)y * tw + x0;
    f4 top;
    if (PLAN && seq_skips(a, seq)) {   // copy-forward: the keyframe's four top-level values
        top = __builtin_nontemporal_load(reinterpret_cast<const f4*>(a.ref[0][a.levels - 1] + ot));
    } else {
        const size_t src_off = (size_t)seq * a.src_w * a.src_img_rows + (size_t)(y << a.src_row_shift) * a.src_w + ((size_t)x0 << CULLS);
        RawWords<CULLS> in;
        in.load_gray(a, src_off);
        const f4 gn = *reinterpret_cast<const f4*>(p.gain + (size_t)load_seq_entry(p.seq_pair, seq) * tw * th + (size_t)y * tw + x0);
#pragma unroll
        for (int k = 0; k < 4; k++) top[k] = pass_valid(photo_gray(RESP_LDS ? lut[in.gray8(k)] : resp[in.gray8(k)], gn[k]));
    }
    __builtin_nontemporal_store(top, reinterpret_cast<f4*>(a.dst[0][a.levels - 1] + ot));
    walk_levels<4, 1>(a, a.levels, seq, x0, y, [&](int l, size_t o, int k) { __builtin_nontemporal_store(pass_valid(top[k]), a.dst[0][l] + o); });
}

// k_pyramid_photo: the scalar form, one thread per top-level pixel: 3 / 4 channels (the response is applied to k_ingest's luma, not
// per channel), the widths k_pyramid_raw4's conditions refuse, and (REMAP) every frame of a handle that also undistorts -- the byte
// is gathered through the camera's table as in k_pyramid_remap, the gain is read at the thread's own (x, y) either way.  PLAN: a
// DVO_SEQ_SKIP sequence copies its keyframe's gray forward as k_pyramid<true> does, or (REMAP) writes nothing as k_pyramid_remap_plan.
template <bool PLAN, bool REMAP>
__global__ void __launch_bounds__(256) k_pyramid_photo(PyramidArgs a, PhotoArgs p)
{
    __shared__ float lut[256];
    const int tw = a.w[a.levels - 1], th = a.h[a.levels - 1];
    const int seq = (int)(blockIdx.z * DVO_GRID_SEQ_Y + blockIdx.y);
    if (seq >= a.n_seq) return;   // (uniform per workgroup)
    lut[threadIdx.x] = p.response[(size_t)load_seq_entry(p.seq_cal, seq) * 256 + threadIdx.x];
    __syncthreads();
    const int i = (int)blockIdx.x * 256 + threadIdx.x;
    if (i >= tw * th) return;
    int x, y;
    split_index(i, tw, a.inv_tw, x, y);
    float raw;
    if (PLAN && seq_skips(a, seq)) {
        if constexpr (REMAP) return;   // (writes nothing)
        raw = __builtin_nontemporal_load(a.ref[0][a.levels - 1] + (size_t)seq * tw * th + i);   // copy-forward: the keyframe's gray
    } else {
        const float gain = p.gain[(size_t)load_seq_entry(p.seq_pair, seq) * tw * th + i];
        size_t src_off;
        bool inside = true;
        if constexpr (REMAP) {
            const int si = a.remap[(size_t)load_seq_entry(a.remap_cam, seq) * tw * th + i];
            inside = si >= 0;
            src_off = (size_t)seq * a.src_w * a.src_h + (size_t)(inside ? si : 0);
        } else {
            src_off = (size_t)seq * a.src_w * a.src_img_rows + (size_t)(y << a.src_row_shift) * a.src_w + (x << a.culls);
        }
        raw = inside ? photo_gray(lut[raw_luma8(a, src_off)], gain) : kInvalid;
    }
    walk_levels<1, 0>(a, a.levels, seq, x, y, [&](int l, size_t o, int) {
        __builtin_nontemporal_store((l == a.levels - 1 && a.culls == 0) ? raw : pass_valid(raw), a.dst[0][l] + o);
    });
}

// k_photometric_map: the gain tables, once per set of the calibration or of D.  One thread per top-level pixel per distinct
// (calibration, undistortion camera) pair; grid seq_grid(., n_pair), the pair in place of the sequence.  The one IEEE division.
__global__ void __launch_bounds__(256) k_photometric_map(const float* __restrict__ vignette, const int* __restrict__ pairs, int n_pair,
                                                         int w, int h, int culls, int tw, int th, const int* __restrict__ remap,
                                                         float* __restrict__ gain)
{
    const int pr = (int)(blockIdx.z * DVO_GRID_SEQ_Y + blockIdx.y);
    const int i = (int)blockIdx.x * 256 + threadIdx.x;
    if (i >= tw * th || pr >= n_pair) return;
    const int cal = pairs[2 * pr], cam = pairs[2 * pr + 1];
    const int y = i / tw, x = i - y * tw;
    const int si = remap ? remap[(size_t)cam * tw * th + i] : (y << culls) * w + (x << culls);
    float out = kPhotoMasked;
    if (si >= 0) {
        const float V = vignette ? vignette[(size_t)cal * w * h + si] : 1.0f;
        if (V > 0.0f && V < __builtin_inff()) out = 1.0f / V;   // (NaN fails both tests)
    }
    gain[(size_t)pr * tw * th + i] = out;
}

// The split build of a big batch's plain raw frames (u8 gray + u16 depth, no plan, no remap): k_pyramid_raw4 as two
// kernels that together write exactly what it writes, from the same conversions and pass_valid calls on the same values.  The
// tracker's coarse levels read only the new frame's gray below the top, so that part is built first on the tracking stream (stage
// A, a quarter of the input rows) and everything else on the low-priority side stream beside the coarse-level launches (stage B).
//
// k_pyramid_raw4_coarse (stage A): the gray maps of every level below the top.  A thread owns four consecutive pixels of level
// top - 1 = top-level pixels (2 lx, 2 ly): 8 << CULLS source pixels of one kept row in two, their gray and (for the d == 0
// invalidation) depth fetched by 16-byte loads, the four values stored as one dwordx4; levels further down take the pixels whose
// level top - 1 coordinates are multiples of 2^(t - 1).  pyramid_can_split checks the alignment all of this needs.
template <int CULLS>
__global__ void __launch_bounds__(256) k_pyramid_raw4_coarse(PyramidArgs a)
{
    const int T = a.levels - 1, cw = a.w[T - 1], ch = a.h[T - 1], gw = cw >> 2;
    const int seq = (int)(blockIdx.z * DVO_GRID_SEQ_Y + blockIdx.y);
    const int gi = (int)blockIdx.x * 256 + threadIdx.x;
    if (gi >= gw * ch || seq >= a.n_seq) return;
    int y, xg;
    split_index(gi, gw, a.inv_tw * 8.0f, xg, y);   // (8 / tw = 1 / gw up to an ulp: split_index corrects +-1)
    const int x0 = xg << 2;                        // level top - 1 coordinates (x0 .. x0 + 3, y)
    const size_t src_off = (size_t)seq * a.src_w * a.src_img_rows + (size_t)((2 * y) << a.src_row_shift) * a.src_w + ((size_t)x0 << (CULLS + 1));
    RawWords<CULLS + 1> in;   // (every second kept pixel of the row)
    in.load_gray(a, src_off);
    in.load_depth(a, src_off);
    f4 g;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        g[k] = pass_valid(raw_convert(a, in.gray8(k), in.depth16(k)).gray);   // (depth and sigma are stage B's)
    }
    __builtin_nontemporal_store(g, reinterpret_cast<f4*>(a.dst[0][T - 1] + (size_t)seq * cw * ch + (size_t)y * cw + x0));
    // the levels below top - 1: the walk of a pyramid whose top is level top - 1
    walk_levels<4, 1>(a, T, seq, x0, y, [&](int l, size_t o, int k) { __builtin_nontemporal_store(g[k], a.dst[0][l] + o); });
}

// k_pyramid_raw4_rest (stage B): k_pyramid_raw4<CULLS, false> with depth, minus the gray stores below the top.  It runs beside
// k_track_gn, which allocates 80 of a lane's 512 registers six times over: 32 registers are left, and this kernel is held to them
// (amdgpu_num_vgpr(32); both instances compile to 26 VGPRs, 0 AGPRs and no scratch: -Rpass-analysis=kernel-resource-usage), so a
// wave of it can become resident without displacing a tracking wave.
template <int CULLS>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_num_vgpr(32))) k_pyramid_raw4_rest(PyramidArgs a)
{
    const int tw = a.w[a.levels - 1], th = a.h[a.levels - 1], gw = tw >> 2;
    const int seq = (int)(blockIdx.z * DVO_GRID_SEQ_Y + blockIdx.y);
    const int gi = (int)blockIdx.x * 256 + threadIdx.x;
    if (gi >= gw * th || seq >= a.n_seq) return;
    int y, xg;
    split_index(gi, gw, a.inv_tw * 4.0f, xg, y);
    const int x0 = xg << 2;
    const size_t src_off = (size_t)seq * a.src_w * a.src_img_rows + (size_t)(y << a.src_row_shift) * a.src_w + ((size_t)x0 << CULLS);
    RawWords<CULLS> in;
    in.load_gray(a, src_off);
    in.load_depth(a, src_off);
    const bool prep = a.wgt[0] != nullptr;
    f4 v[3];   // pass_valid of gray, depth, sigma of the four kept pixels: what every level stores
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const RawPixel p = raw_convert(a, in.gray8(k), in.depth16(k));
        v[0][k] = pass_valid(p.gray); v[1][k] = pass_valid(p.depth); v[2][k] = pass_valid(p.sigma);
    }
    {
        const int l = a.levels - 1;
        const size_t o = (size_t)seq * tw * th + (size_t)y * tw + x0;
        __builtin_nontemporal_store(v[0], reinterpret_cast<f4*>(a.dst[0][l] + o));
        if (a.dst[1][l]) __builtin_nontemporal_store(v[1], reinterpret_cast<f4*>(a.dst[1][l] + o));
        if (a.dst[2][l]) __builtin_nontemporal_store(v[2], reinterpret_cast<f4*>(a.dst[2][l] + o));
        if (prep) {
            f4 wgv;
#pragma unroll
            for (int k = 0; k < 4; k++) wgv[k] = gn_weight(a.step[l], a.sigma_min, a.sigma_max, v[2][k]);
            __builtin_nontemporal_store(wgv, reinterpret_cast<f4*>(a.wgt[l] + o));
        }
    }
    // walk_levels<4, 1> written out: under the helper this kernel measured 3 % slower beside k_track_gn.  Stage A
    // has written the gray below the top.
    for (int t = 1; t < a.levels; t++) {
        const int msk = (1 << t) - 1;
        if (y & msk) break;
        const int l = a.levels - 1 - t, ly = y >> t;
        if (ly >= a.h[l]) continue;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int x = x0 + k;
            if (x & msk) continue;
            const int lx = x >> t;
            if (lx >= a.w[l]) continue;
            const size_t o = (size_t)seq * a.w[l] * a.h[l] + (size_t)ly * a.w[l] + lx;
            if (a.dst[1][l]) __builtin_nontemporal_store(v[1][k], a.dst[1][l] + o);
            if (a.dst[2][l]) __builtin_nontemporal_store(v[2][k], a.dst[2][l] + o);
            if (prep) __builtin_nontemporal_store(gn_weight(a.step[l], a.sigma_min, a.sigma_max, v[2][k]), a.wgt[l] + o);
        }
    }
}

// k_pyramid_remap_depth: k_pyramid of SENSOR-DEPTH frames (gray + depth + sigma, float maps or raw u8 gray/RGB(A) + u16 depth)
// with the lens undistortion fused in (dvo_batch_set_sensor_distortion).  As k_pyramid_remap, kept pixel (x << culls, y << culls)
// of the undistorted frame is ONE source pixel: the thread reads its index from the sequence's camera table (k_undistort_map, -1 =
// border) and gathers gray, depth and sigma (raw: the u8 gray / RGB(A) and the u16 depth) from that one index.  The conversions
// are per pixel, so they commute with the gather: k_pyramid's raw conversion applied to the gathered bytes gives the bits of
// dvo_op_undistort applied to each of dvo_op_ingest's three maps.  A border pixel is DVO_INVALID in all three maps, as
// dvo_op_undistort writes it (its depth, -2, is below any min_depth: it never contributes).  Every level and the fused wgt maps are
// written with k_pyramid's operations.  PPT = 4 (the usual case: tw % 4 == 0, 16-byte aligned tops and table) reads four table
// entries with one 16-byte load and writes the four top-level values of each map with one 16-byte store, as k_pyramid_raw4;
// PPT = 1 is the scalar fallback.  PLAN: the workgroups of a DVO_SEQ_SKIP sequence copy their reference forward, as k_pyramid<true>.
// The table is read with plain loads (one table serves every sequence of the camera and stays in L2), the frames and the levels
// with nontemporal accesses.  The input holds whole frames (src_img_rows = src_h): the gather reads any row.
template <int PPT, bool PLAN>
__global__ void __launch_bounds__(256) k_pyramid_remap_depth(PyramidArgs a)
{
    static_assert(PPT == 1 || PPT == 4, "one or four kept pixels per thread");
    const int tw = a.w[a.levels - 1], th = a.h[a.levels - 1], gw = tw / PPT;
    const int seq = (int)(blockIdx.z * DVO_GRID_SEQ_Y + blockIdx.y);
    const int gi = (int)blockIdx.x * 256 + threadIdx.x;
    if (gi >= gw * th || seq >= a.n_seq) return;
    int y, xg;
    split_index(gi, gw, a.inv_tw * (float)PPT, xg, y);
    const int x0 = xg * PPT, T = a.levels - 1;
    const size_t ot = (size_t)seq * tw * th + (size_t)y * tw + x0;
    const bool prep = a.wgt[0] != nullptr;   // (depth and sigma are always present here)
    bool skip = false;
    if constexpr (PLAN) skip = seq_skips(a, seq);
    float top[3][PPT];   // the top-level value of each map: what the build stores there (lower levels: pass_valid of it)
#pragma unroll
    for (int m = 0; m < 3; m++)
#pragma unroll
        for (int k = 0; k < PPT; k++) top[m][k] = 0.0f;
    if (skip) {   // copy-forward: every value this thread's build would write, none of its input
#pragma unroll
        for (int m = 0; m < 3; m++) {
            if (a.dst[m][T] == nullptr) continue;
            if constexpr (PPT == 4) {
                const f4 v = __builtin_nontemporal_load(reinterpret_cast<const f4*>(a.ref[m][T] + ot));
                top[m][0] = v.x; top[m][1] = v.y; top[m][2] = v.z; top[m][3] = v.w;
            } else {
                top[m][0] = __builtin_nontemporal_load(a.ref[m][T] + ot);
            }
        }
    } else {
        const int cam = load_seq_entry(a.remap_cam, seq);   // (one scalar load)
        const int* tab = a.remap + (size_t)cam * tw * th + (size_t)y * tw + x0;
        int si[PPT];
        if constexpr (PPT == 4) {
            const i32x4 e = *reinterpret_cast<const i32x4*>(tab);
            si[0] = e.x; si[1] = e.y; si[2] = e.z; si[3] = e.w;
        } else {
            si[0] = tab[0];
        }
        const size_t base = (size_t)seq * a.src_w * a.src_h;
#pragma unroll
        for (int k = 0; k < PPT; k++) {
            float raw[3] = {kInvalid, kInvalid, kInvalid};
            if (si[k] >= 0) {
                const size_t so = base + (size_t)si[k];
                if (a.raw_rgb != nullptr) {   // the raw conversion of the one gathered pixel
                    const RawPixel p = raw_convert(a, raw_luma8(a, so), __builtin_nontemporal_load(a.raw_depth + so));
                    raw[0] = p.gray; raw[1] = p.depth; raw[2] = p.sigma;
                } else {
#pragma unroll
                    for (int m = 0; m < 3; m++) raw[m] = __builtin_nontemporal_load(a.src[m] + so);
                }
            }
            // top level: cullImage(src, culls); culls == 0 aliases the input (convert.cpp:9-10), no pass_valid
#pragma unroll
            for (int m = 0; m < 3; m++) top[m][k] = a.culls == 0 ? raw[m] : pass_valid(raw[m]);
        }
    }
    // top level (t = 0)
    if constexpr (PPT == 4) {
#pragma unroll
        for (int m = 0; m < 3; m++)
            if (a.dst[m][T] != nullptr)
                __builtin_nontemporal_store(f4{top[m][0], top[m][1], top[m][2], top[m][3]}, reinterpret_cast<f4*>(a.dst[m][T] + ot));
        if (prep) {
            f4 wgv;
            if (skip) {
                wgv = __builtin_nontemporal_load(reinterpret_cast<const f4*>(a.ref_wgt[T] + ot));
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++) wgv[k] = gn_weight(a.step[T], a.sigma_min, a.sigma_max, top[2][k]);
            }
            __builtin_nontemporal_store(wgv, reinterpret_cast<f4*>(a.wgt[T] + ot));
        }
    } else {
#pragma unroll
        for (int m = 0; m < 3; m++)
            if (a.dst[m][T] != nullptr) __builtin_nontemporal_store(top[m][0], a.dst[m][T] + ot);
        if (prep)
            __builtin_nontemporal_store(skip ? __builtin_nontemporal_load(a.ref_wgt[T] + ot) : gn_weight(a.step[T], a.sigma_min, a.sigma_max, top[2][0]),
                                        a.wgt[T] + ot);
    }
    walk_levels<PPT, 1>(a, a.levels, seq, x0, y, [&](int l, size_t o, int k) {
        const float sg = pass_valid(top[2][k]);
#pragma unroll
        for (int m = 0; m < 3; m++)
            if (a.dst[m][l] != nullptr) __builtin_nontemporal_store(m == 2 ? sg : pass_valid(top[m][k]), a.dst[m][l] + o);
        if (prep)
            __builtin_nontemporal_store(skip ? __builtin_nontemporal_load(a.ref_wgt[l] + o) : gn_weight(a.step[l], a.sigma_min, a.sigma_max, sg),
                                        a.wgt[l] + o);
    });
}

// ------------------------------------------------------------------------------------------------
// The binomial-filtered gray pyramid of a sensor-depth batch (dvo_batch_set_pyramid_filter, DVO_PYRAMID_FILTER_BINOMIAL3;
// include/dvo.h states the contract, DESIGN.md §39 the design).  Gray only: depth, sigma and wgt are the plain build's values.
// ------------------------------------------------------------------------------------------------
// One tap of a halving: an invalid tap (NaN, <= kInvalid; a tap outside the map is held as kInvalid) is skipped
__device__ __forceinline__ void filter_tap(float g, int k, float& S, int& W)
{
    if (is_valid(g)) { S = fmaf((float)k, g, S); W += k; }
}

// One halving H at centre tap c[0] of a map with `pitch` floats per row whose 3x3 neighbourhood is readable: rows j = -1, 0, 1
// outside, columns i = -1, 0, 1 inside, weights (2 - |i|)(2 - |j|), one division
__device__ __forceinline__ float filter_halve(const float* c, int pitch)
{
    if (!is_valid(c[0])) return kInvalid;
    float S = 0.0f;
    int W = 0;
#pragma unroll
    for (int j = -1; j <= 1; j++)
#pragma unroll
        for (int i = -1; i <= 1; i++) filter_tap(c[j * pitch + i], (2 - (i < 0 ? -i : i)) * (2 - (j < 0 ? -j : j)), S, W);
    return S / (float)W;
}

// The converted source gray G0 of pixel `off` of a whole input frame: raw_convert's gray (kInvalid where the depth word is 0) or
// the float map's value
template <bool RAW>
__device__ __forceinline__ float filter_source_gray(const PyramidArgs& a, size_t off)
{
    if constexpr (RAW) {
        const unsigned d = a.raw_depth != nullptr ? (unsigned)__builtin_nontemporal_load(a.raw_depth + off) : 1u;
        return raw_convert(a, raw_luma8(a, off), d).gray;
    } else {
        return __builtin_nontemporal_load(a.src[0] + off);
    }
}

// k_pyramid_filter_top: the top level of every map, and depth / sigma / wgt of every level.  A workgroup owns a 32 x 8 tile of
// the top level.  It stages the tile's footprint of G0 (the tile << CULLS plus 2^CULLS - 1 rows and columns ahead of it: 3 x 3
// per halving) in LDS, out-of-frame pixels as kInvalid, reduces it there (CULLS = 2: through the 65 x 17 intermediate tile, also
// in LDS; no map at source or intermediate resolution exists in memory), and each thread stores its pixel.  Depth and sigma are
// read at the kept pixel and stored at every level with k_pyramid's operations.  CULLS = 0: the top level is the input.
// WIDE: the footprint is staged in 16-byte loads (16 raw pixels: one gray and two depth loads, or 4 float pixels), from a
// 16-byte aligned column ahead of the tile; needs 1-channel bytes, src_w a multiple of the chunk and 16-byte aligned inputs
// (pyramid_filter_wide).  Otherwise one pixel per load.  The input holds whole frames.
// PLAN: the workgroups of a DVO_SEQ_SKIP sequence copy the reference's top-level values forward as k_pyramid<true> does
// (k_pyramid_filter_down<true> copies the gray of the lower levels).
template <int CULLS, bool RAW, bool PLAN, bool WIDE>
__global__ void __launch_bounds__(256) k_pyramid_filter_top(PyramidArgs a)
{
    static_assert(CULLS >= 0 && CULLS <= 2 && !(WIDE && CULLS == 0), "culls 0 stages nothing");
    constexpr int TX = 32, TY = 8;
    constexpr int HALO = (1 << CULLS) - 1;
    constexpr int C = WIDE ? (RAW ? 16 : 4) : 1;     // pixels per staging load
    constexpr int LEFT = WIDE ? C : HALO;            // columns staged ahead of the tile's first source column
    constexpr int SW = (TX << CULLS) + LEFT, SH = (TY << CULLS) + HALO;
    constexpr int IW = 2 * TX + 1, IH = 2 * TY + 1;  // the intermediate tile of CULLS = 2
    __shared__ __attribute__((aligned(16))) float s_src[CULLS > 0 ? SH * SW : 4];
    __shared__ float s_mid[CULLS == 2 ? IH * IW : 1];
    const int T = a.levels - 1, tw = a.w[T], th = a.h[T];
    const int seq = (int)(blockIdx.z * DVO_GRID_SEQ_Y + blockIdx.y);
    if (seq >= a.n_seq) return;
    const int tiles_x = (tw + TX - 1) / TX;
    const int by = (int)blockIdx.x / tiles_x, bx = (int)blockIdx.x - by * tiles_x;
    const int X0 = bx * TX, Y0 = by * TY;
    const int tx = threadIdx.x & (TX - 1), ty = threadIdx.x / TX;
    const int x = X0 + tx, y = Y0 + ty;
    bool skip = false;
    if constexpr (PLAN) skip = seq_skips(a, seq);   // (uniform per workgroup: the barriers below are too)
    const size_t base = (size_t)seq * a.src_w * a.src_h;
    float gray = kInvalid;
    if constexpr (CULLS > 0) if (!skip) {
        const int sx0 = (X0 << CULLS) - LEFT, sy0 = (Y0 << CULLS) - HALO;
        constexpr int CPR = SW / C;
        for (int i = threadIdx.x; i < SH * CPR; i += 256) {
            const int r = i / CPR, c = (i - r * CPR) * C;
            const int sy = sy0 + r, sx = sx0 + c;
            const bool in = sy >= 0 && sy < a.src_h && sx >= 0 && sx < a.src_w;   // (WIDE: src_w % C == 0, a chunk is in or out whole)
            const size_t off = base + (size_t)sy * a.src_w + sx;
            float* out = s_src + r * SW + c;
            if constexpr (!WIDE) {
                out[0] = in ? filter_source_gray<RAW>(a, off) : kInvalid;
            } else if constexpr (RAW) {
                f4 v[4];
#pragma unroll
                for (int q = 0; q < 4; q++) v[q] = f4{kInvalid, kInvalid, kInvalid, kInvalid};
                if (in) {
                    const u32x4 g = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(a.raw_rgb + off));
                    u32x4 d[2] = {u32x4{0x00010001u, 0x00010001u, 0x00010001u, 0x00010001u}, u32x4{0x00010001u, 0x00010001u, 0x00010001u, 0x00010001u}};
                    if (a.raw_depth != nullptr) {
                        d[0] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(a.raw_depth + off));
                        d[1] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(a.raw_depth + off) + 1);
                    }
#pragma unroll
                    for (int k = 0; k < 16; k++) {
                        const unsigned g8 = (g[k >> 2] >> ((k & 3) * 8)) & 0xffu;
                        const unsigned dk = (d[k >> 3][(k >> 1) & 3] >> ((k & 1) * 16)) & 0xffffu;
                        v[k >> 2][k & 3] = raw_convert(a, g8, dk).gray;
                    }
                }
#pragma unroll
                for (int q = 0; q < 4; q++) reinterpret_cast<f4*>(out)[q] = v[q];
            } else {
                f4 v = f4{kInvalid, kInvalid, kInvalid, kInvalid};
                if (in) v = __builtin_nontemporal_load(reinterpret_cast<const f4*>(a.src[0] + off));
                *reinterpret_cast<f4*>(out) = v;
            }
        }
        __syncthreads();
        if constexpr (CULLS == 2) {
            const int mx0 = 2 * X0 - 1, my0 = 2 * Y0 - 1, mw = a.src_w >> 1, mh = a.src_h >> 1;
            for (int i = threadIdx.x; i < IH * IW; i += 256) {
                const int r = i / IW, c = i - r * IW;
                const int mx = mx0 + c, my = my0 + r;
                float v = kInvalid;   // (outside the intermediate map: skipped by the second halving)
                if (mx >= 0 && mx < mw && my >= 0 && my < mh) v = filter_halve(s_src + (2 * my - sy0) * SW + (2 * mx - sx0), SW);
                s_mid[i] = v;
            }
            __syncthreads();
            gray = filter_halve(s_mid + (2 * ty + 1) * IW + (2 * tx + 1), IW);
        } else {
            gray = filter_halve(s_src + (2 * y - sy0) * SW + (2 * x - sx0), SW);
        }
    }
    if (x >= tw || y >= th) return;
    bool have[3];
    have[0] = true;
    if constexpr (RAW) have[1] = have[2] = a.raw_depth != nullptr;
    else { have[1] = a.src[1] != nullptr; have[2] = a.src[2] != nullptr; }
    const bool prep = a.wgt[0] != nullptr && have[1] && have[2];
    const size_t ot = (size_t)seq * tw * th + (size_t)y * tw + x;
    float top[3] = {0.0f, 0.0f, 0.0f};
    if (skip) {
#pragma unroll
        for (int m = 0; m < 3; m++)
            if (have[m] && a.dst[m][T] != nullptr) top[m] = __builtin_nontemporal_load(a.ref[m][T] + ot);
    } else {
        const size_t so = base + (size_t)(y << CULLS) * a.src_w + (x << CULLS);
        float raw[3] = {0.0f, 0.0f, 0.0f};
        if constexpr (RAW) {
            if (have[1]) {
                const RawPixel p = raw_convert(a, 0u, __builtin_nontemporal_load(a.raw_depth + so));
                raw[1] = p.depth; raw[2] = p.sigma;
            }
        } else {
#pragma unroll
            for (int m = 1; m < 3; m++)
                if (have[m]) raw[m] = __builtin_nontemporal_load(a.src[m] + so);
        }
        // top level: cullImage(src, culls); culls == 0 aliases the input (convert.cpp:9-10), no pass_valid
        if constexpr (CULLS == 0) raw[0] = filter_source_gray<RAW>(a, so);
        top[0] = CULLS == 0 ? raw[0] : gray;
        top[1] = CULLS == 0 ? raw[1] : pass_valid(raw[1]);
        top[2] = CULLS == 0 ? raw[2] : pass_valid(raw[2]);
    }
    if (a.dst[0][T] != nullptr) __builtin_nontemporal_store(top[0], a.dst[0][T] + ot);
    walk_levels<1, 0>(a, a.levels, seq, x, y, [&](int l, size_t o, int) {
        float val[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int m = 1; m < 3; m++) {
            val[m] = l == T ? top[m] : pass_valid(top[m]);
            if (have[m] && a.dst[m][l] != nullptr) __builtin_nontemporal_store(val[m], a.dst[m][l] + o);
        }
        if (prep)
            __builtin_nontemporal_store(skip ? __builtin_nontemporal_load(a.ref_wgt[l] + o) : gn_weight(a.step[l], a.sigma_min, a.sigma_max, val[2]),
                                        a.wgt[l] + o);
    });
}

// k_pyramid_filter_down: gray of level l = H(stored gray of level l + 1), one thread per pixel of level l, one launch per level
// below the top (each reads what the launch before it stored; the nine taps of neighbouring threads overlap in L2).
// PLAN: a DVO_SEQ_SKIP sequence copies the reference's gray of level l.
template <bool PLAN>
__global__ void __launch_bounds__(256) k_pyramid_filter_down(PyramidArgs a, int l, float inv_w)
{
    const int w = a.w[l], h = a.h[l], iw = a.w[l + 1], ih = a.h[l + 1];
    const int seq = (int)(blockIdx.z * DVO_GRID_SEQ_Y + blockIdx.y);
    const int i = (int)blockIdx.x * 256 + threadIdx.x;
    if (i >= w * h || seq >= a.n_seq) return;
    const size_t o = (size_t)seq * w * h + i;
    if constexpr (PLAN) {
        if (seq_skips(a, seq)) {
            __builtin_nontemporal_store(__builtin_nontemporal_load(a.ref[0][l] + o), a.dst[0][l] + o);
            return;
        }
    }
    int x, y;
    split_index(i, w, inv_w, x, y);
    const float* in = a.dst[0][l + 1] + (size_t)seq * iw * ih;
    float out = kInvalid;
    if (is_valid(in[(size_t)(2 * y) * iw + 2 * x])) {
        float S = 0.0f;
        int W = 0;
#pragma unroll
        for (int j = -1; j <= 1; j++)
#pragma unroll
            for (int k = -1; k <= 1; k++) {
                const int xx = 2 * x + k, yy = 2 * y + j;
                if (xx < 0 || xx >= iw || yy < 0 || yy >= ih) continue;
                filter_tap(in[(size_t)yy * iw + xx], (2 - (k < 0 ? -k : k)) * (2 - (j < 0 ? -j : j)), S, W);
            }
        out = S / (float)W;
    }
    __builtin_nontemporal_store(out, a.dst[0][l] + o);
}

// k_cull: a single Convert::cullImage (operator-level parity)
__global__ void __launch_bounds__(256) k_cull(const float* __restrict__ src, int w, int h, int times, float* __restrict__ dst)
{
    const int dw = w >> times, dh = h >> times;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= dw * dh) return;
    const int y = i / dw, x = i - y * dw;
    const float raw = src[(size_t)(y << times) * w + (x << times)];
    dst[i] = times > 0 ? pass_valid(raw) : raw;
}

// k_gradient: Convert::gradiate (convert.cpp:41-75), standalone parity op
__global__ void __launch_bounds__(256) k_gradient(const float* __restrict__ img, int w, int h, int xdir, float* __restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= w * h) return;
    const int y = i / w, x = i - y * w;
    GlobalImg g{img, w, h};
    out[i] = xdir ? grad_x_at(g, x, y) : grad_y_at(g, x, y);
}

// k_warp_image: Transform::warpImage (transform.cpp:35-51), standalone parity/visual op.  The fused tracker
// never materialises this image.
__global__ void __launch_bounds__(256) k_warp_image(const float* __restrict__ gray, const float* __restrict__ depth,
                                                    int w, int h, Intr k, Pose pose, float* __restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= w * h) return;
    const int y = i / w, x = i - y * w;
    const float d = depth[i];
    float v = kInvalid;
    if (!is_epsilon(d)) {
        float pu, pv;
        warp(pose, k, (float)x, (float)y, d, pu, pv);
        GlobalImg g{gray, w, h};
        v = get_subpixel(g, pu, pv);
    }
    out[i] = v;
}

// ------------------------------------------------------------------------------------------------
// k_track_gn: the fused Gauss-Newton accumulation = Transform::warpImage + Track::optimize's per-pixel
// lambda (optimize.cpp:28-90) + the A^T A / A^T B products that cv::solve's SVD stands for.
//
// HBM traffic per evaluated pixel, by contract: obj_gray 4 + ref_depth 4 + ref_sigma 4 (coalesced rows) + ref_gray 4
// (12-tap plus-shaped gather around the warped position, served by L1/L2 or the LDS patch) = 16 B.  Read in fact: the weight map
// step / clamp(sigma) in place of sigma -- or nothing at all for raw sensor frames, whose contributing pixels share one weight
// (GnArgs::wgt_const) -- and 1 / depth recomputed (recip_gated): 12-13 B.  Through the L1 it is 56 B per lane and pixel (8 B of rows,
// 48 B of taps), and that path, 78 % busy, limits the kernel together with the vector ALUs.
// Each thread owns PPT pixels (stride 256 => coalesced), keeps 29 accumulators (21 upper-tri J^T J, 6 J^T wr,
// sum r^2, count), then: DPP wave sum -> LDS across the 4 waves -> one 32-float partial per workgroup.
// ------------------------------------------------------------------------------------------------
// 1.0f / d for the lanes that pass the gates of optimize.cpp:33-48 (d >= min_depth > 0), the IEEE quotient bit for bit: the
// v_rcp_f32 + two-FMA form of dvo_math.h wherever it is proven equal to the division (|d| in [2^-100, 2^100], all floats compared
// on the device), the division itself for the wave when a gated lane lies outside.  Lanes that fail the gate get an unspecified
// finite-or-not value: their Jacobian row is replaced by zeros (a select, not a product) before it is used.
__device__ __forceinline__ float recip_gated(float d, bool gate)
{
#if defined(__HIP_DEVICE_COMPILE__)
    float r = recip_fast(d);
    const float ad = fabsf(d);
    const bool odd = gate & !((ad >= DVO_RECIP_FAST_MIN) & (ad <= DVO_RECIP_FAST_MAX));   // (true for NaN; min_depth is configurable)
    if (__builtin_amdgcn_ballot_w64(odd) != 0ull) {       // wave-uniform; never taken for a real depth map
        asm volatile("; recip_gated: IEEE division fallback");
        if (odd) r = 1.0f / d;
    }
    return r;
#else
    (void)gate;
    return 1.0f / d;
#endif
}

struct Acc29 {
    float a[29];
    __device__ __forceinline__ void zero()
    {
#pragma unroll
        for (int i = 0; i < 29; i++) a[i] = 0.0f;
    }
    __device__ __forceinline__ void add(const float J[6], float r, float rw, float one)
    {
        int idx = 0;
#pragma unroll
        for (int p = 0; p < 6; p++)
#pragma unroll
            for (int q = p; q < 6; q++) {
                a[idx] = fmaf(J[p], J[q], a[idx]);
                idx++;
            }
#pragma unroll
        for (int p = 0; p < 6; p++) a[21 + p] = fmaf(J[p], rw, a[21 + p]);
        a[27] = fmaf(r, r, a[27]);
        a[28] += one;
    }
    // the weighted sums of DESIGN.md §23: Jr = rho * J (one rounded multiply), then the slots and fmaf shape of add(); rho = 1 gives add()'s bits
    __device__ __forceinline__ void add_w(const float J[6], float r, float rw, float one, float rho)
    {
        float Jr[6];
#pragma unroll
        for (int p = 0; p < 6; p++) Jr[p] = rho * J[p];
        int idx = 0;
#pragma unroll
        for (int p = 0; p < 6; p++)
#pragma unroll
            for (int q = p; q < 6; q++) {
                a[idx] = fmaf(Jr[p], J[q], a[idx]);
                idx++;
            }
#pragma unroll
        for (int p = 0; p < 6; p++) a[21 + p] = fmaf(Jr[p], rw, a[21 + p]);
        a[27] = fmaf(rho * r, r, a[27]);
        a[28] += one;
    }
};

// dword-aligned wide loads (gfx950 global memory takes unaligned dwordx2/x4)
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
typedef float f2u __attribute__((ext_vector_type(2), aligned(4)));

// the generic sampler as a real function: rare (border / INVALID taps), keeps the hot loop's code small
struct SlowSample {  // returned in registers (an out-pointer would put the caller's locals in scratch memory)
    float I2, gx, gy;
    int ok;
};
__device__ __noinline__ SlowSample gn_sample_slow(const float* img, int w, int h, float d, float u, float v)
{
    const GlobalImg ref{img, w, h};
    SlowSample s;
    s.ok = gn_sample(ref, d, u, v, s.I2, s.gx, s.gy) ? 1 : 0;
    return s;
}

// The 12 plus-shaped taps around (x0, y0) that warped gray (4 taps) and its central-difference gradient need.
struct Taps {
    f2u ra;  // row y0-1: cols x0, x0+1
    f4u rb;  // row y0  : cols x0-1 .. x0+2
    f4u rc;  // row y0+1: cols x0-1 .. x0+2
    f2u rd;  // row y0+2: cols x0, x0+1
};

// Interior fast path.  When the 4x4 neighbourhood of the warped position lies inside the image and its 12 taps are
// all valid, getSubpixel's fill loop is a no-op and Convert::gradiate has no border/invalid case, so warped gray
// and gradient reduce to straight differences and three blend4() calls -- the SAME float operations the generic
// path (dvo_math.h gn_sample) performs, without its per-tap branches.  Returns 1 = sampled, 0 = pixel rejected,
// -1 = not decidable here (INVALID or NaN tap): take the generic path.
// v_min3_f32 without the canonicalising v_max that fminf() adds to every loaded operand.  NaN operands are either
// skipped (caught by the probe below) or returned (fails the > test): both end in the generic path.
__device__ __forceinline__ float min3_raw(float a, float b, float c)
{
    float m;
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(m) : "v"(a), "v"(b), "v"(c));
    return m;
}

__device__ __forceinline__ void gn_sample_fast(const Taps& t, float u, float v, int x0, int y0, float& I2, float& gx, float& gy,
                                               bool& decidable, bool& valid)
{  // branch free: everything is computed; decidable = no INVALID / NaN tap (else: generic path), valid = pixel contributes
    const float mn = min3_raw(min3_raw(min3_raw(t.ra.x, t.ra.y, t.rd.x), min3_raw(t.rb.x, t.rb.y, t.rb.z), min3_raw(t.rc.x, t.rc.y, t.rc.z)),
                              min3_raw(t.rd.y, t.rb.w, t.rc.w), t.rd.y);
    const float hx = u - (float)x0, vy = v - (float)y0;   // (v_fract_f32 gives the same bits for u >= 1 and saves two conversions: measured, no gain)
    I2 = blend4(t.rb.y, t.rb.z, t.rc.y, t.rc.z, hx, vy);
    gx = blend4(t.rb.z - t.rb.x, t.rb.w - t.rb.y, t.rc.z - t.rc.x, t.rc.w - t.rc.y, hx, vy);
    gy = blend4(t.rc.y - t.ra.x, t.rc.z - t.ra.y, t.rd.x - t.rb.y, t.rd.y - t.rb.z, hx, vy);
    const float probe = (I2 + gx) + gy;  // a NaN tap (fminf skips NaN) poisons at least one of the three
    decidable = (mn > kInvalid) & (probe == probe);
    valid = ((int)is_invalid(I2) | (int)is_invalid(gx) | (int)is_invalid(gy)) == 0;  // bitwise on purpose: no short-circuit branches
}

// The generic sampler (dvo_math.h gn_sample: any position, any validity pattern -- the fill quirk of getSubpixel, INVALID gradients at the
// image border and next to INVALID taps, clamping of missing taps to g00) with every tap it can touch requested UP FRONT from clamped
// coordinates: one memory round trip instead of the five or six dependent ones of the branchy version, its semantics then evaluated from
// registers with selects.  Written for k_track_persist, where every step waits for its slowest tile and the slowest tiles are those with
// border pixels (5.3-6.1 us against 2.85 us for an interior tile: 6.1 -> 5.0 us, profiles/r03_single_cpp_final.txt); then measured in
// the throughput kernels as well: +3.0 % frames/s on the 16 384-sequence batch (311.5 k -> 320.8 k, profiles/r03_patch_sampler_ab.txt) --
// a round-1 attempt of the same idea had been 20 % slower on the probe and was the reason the branchy version stayed this long.
// The same float operations on the same values: bit-identical results (tests/test_gpu_parity.py: operator-level masks against the
// oracle, the schedules against each other, frames full of INVALID blocks, black pixels and depth holes).
__device__ __forceinline__ bool gn_sample_patch(const float* __restrict__ img, const int w, const int h, const float d, const float u, const float v,
                                                float& I2, float& gx, float& gy)
{
    I2 = kInvalid; gx = kInvalid; gy = kInvalid;
    if (is_epsilon(d) || !coord_ok(u) || !coord_ok(v)) return false;   // transform.cpp:44; load_taps' first gate
    const int x0 = (int)u, y0 = (int)v;
    if (x0 < 0 || w <= x0 || y0 < 0 || h <= y0) return false;
    const bool hasXm = x0 >= 1, inx = x0 + 1 < w, hasX2 = x0 + 2 < w, hasYm = y0 >= 1, iny = y0 + 1 < h, hasY2 = y0 + 2 < h;
    const int xm = hasXm ? x0 - 1 : x0, x1 = inx ? x0 + 1 : x0, x2 = hasX2 ? x0 + 2 : x0;
    const int rm = (hasYm ? y0 - 1 : y0) * w, r0 = y0 * w, r1 = (iny ? y0 + 1 : y0) * w, r2 = (hasY2 ? y0 + 2 : y0) * w;
    const float Tm0 = img[rm + x0], Tm1 = img[rm + x1];
    const float T0m = img[r0 + xm], T00 = img[r0 + x0], T01 = img[r0 + x1], T02 = img[r0 + x2];
    const float T1m = img[r1 + xm], T10 = img[r1 + x0], T11 = img[r1 + x1], T12 = img[r1 + x2];
    const float T20 = img[r2 + x0], T21 = img[r2 + x1];
    const float hx = u - (float)x0, vy = v - (float)y0;
    float g[4] = {T00, inx ? T01 : T00, iny ? T10 : T00, (inx && iny) ? T11 : T00};   // load_taps: a missing tap is g00
    if (!fill_quirk(g)) return false;
    I2 = blend4(g[0], g[1], g[2], g[3], hx, vy);
    if (is_invalid(I2)) return false;
    if (u < 0.0f || v < 0.0f || (float)w <= u || (float)h <= v) return false;       // optimize.cpp:52-56
    // Convert::gradiate at the four corners (grad_x_at / grad_y_at): INVALID unless both neighbours exist and are valid
    auto diff = [](bool exists, float a, float b) { return (exists && is_valid(a) && is_valid(b)) ? b - a : kInvalid; };
    const float gx00 = diff(hasXm && inx, T0m, T01);
    const float gx10 = inx ? diff(hasX2, T00, T02) : gx00;
    const float gx01 = iny ? diff(hasXm && inx, T1m, T11) : gx00;
    const float gx11 = (inx && iny) ? diff(hasX2, T10, T12) : gx00;
    const float gy00 = diff(hasYm && iny, Tm0, T10);
    const float gy10 = inx ? diff(hasYm && iny, Tm1, T11) : gy00;
    const float gy01 = iny ? diff(hasY2, T00, T20) : gy00;
    const float gy11 = (inx && iny) ? diff(hasY2, T01, T21) : gy00;
    gx = blend4(gx00, gx10, gx01, gx11, hx, vy);
    gy = blend4(gy00, gy10, gy01, gy11, hx, vy);
    return !(is_invalid(gx) || is_invalid(gy));
}

// k_prep_ref: the per-pixel constant of a reference frame (all levels, one launch): wgt = step(level) / clamp(sigma) -- the
// division of optimize.cpp:83-84, which does not depend on the pose, evaluated once per frame instead of once per Gauss-Newton
// iteration.  (1 / depth, optimize.cpp:70-74, was a second such map in round 1: 4 B per pixel and iteration through HBM and the L1
// for five instructions; the kernels now recompute it -- recip_rn, the IEEE quotient bit for bit.)
__global__ void __launch_bounds__(256) k_prep_ref(PrepArgs a)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.level_end[a.levels - 1]) return;
    float step = a.step[0];
#pragma unroll
    for (int l = 1; l < DVO_MAX_LEVELS; l++)
        if (l < a.levels && i >= a.level_end[l - 1]) step = a.step[l];
    a.wgt[i] = gn_weight(step, a.sigma_min, a.sigma_max, a.sigma[i]);
}

// The intrinsics a tracking kernel uses for its sequence: a.k, or (PCAM: the per-camera instantiations) `cam`, the sequence's entry
// of the per-sequence table GnArgs::seq_k, which the kernel loads once at its start -- ahead of every store and barrier, so the
// 24 bytes (wave-uniform address) arrive by scalar loads into SGPRs.  Called at each use, with a.k not bound to a local: PCAM =
// false is then the very code it always was (binding it, or passing it as a used parameter, reschedules k_track_gn).
template <bool PCAM>
__device__ __forceinline__ const Intr& seq_intr(const GnArgs& a, const Intr& cam)
{
    if constexpr (PCAM) return cam;
    else return a.k;
}

// LDS of one gn_tile() evaluation (the caller owns it: k_track_gn once, k_track_level once per tile and iteration)
template <int PPT>
struct GnTileLds {
    float red[4][32];
    int slow_q[4][PPT * 64];  // deferred pixels (generic sampler), one queue per wave
    int slow_cnt[4];
};

// gn_tile: one 256 x PPT pixel tile (`blk`) of sequence `seq` at pose `pose` -> its 32-float partial row `out_row`
// (global or LDS).  Called by all 256 threads of a workgroup; contains two barriers.
// PCAM: the sequence's own intrinsics `cam` instead of a.k (seq_intr; `cam` is unused otherwise).
// T2D: the tile is 64 columns x 4*PPT rows (lane = column, wave w owns rows w*PPT .. w*PPT+PPT-1) instead of 256*PPT
// consecutive raster pixels.  Used when the level width is a multiple of 64: only tiles on the image border then hold
// deferred (border) pixels, a thread's pixels share their column (one int->float conversion and one (x - cx) for PPT
// pixels) and there is no row-wrap arithmetic.
// ROB: every contributing pixel is weighted by robust_rho(rob, r) (k_track_gn_rw; `rob` is unused otherwise, and ROB = false is the
// code it always was).
// AB: the residual is taken against the compensated brightness fmaf(ab.a, I1, ab.b) and the tile's brightness moments go to mom_row
// through mred (k_track_gn_ab; unused otherwise, and AB = false is the code it always was).
// GEO: a.ref_depth / a.ref_wgt are the tracked frame's own maps, and a contributing pixel of the fast path whose 12 reference-depth
// taps (geo.ref_z, the gray taps' byte offsets) pass the gates adds a geometric row to slots 0..26 and to slots 29 / 30 of the partial
// row, reduced through mred (k_track_gn_z; unused otherwise, and GEO = false is the code it always was).
// MED: every contributing pixel's |r| is counted in its bin of `hist`, the workgroup's 256 LDS counters (k_track_gn_md, DESIGN.md §30;
// with ROB only; unused otherwise, and MED = false is the code it always was).  The caller clears and flushes `hist`.
template <int PPT, int G, bool MASK, bool T2D, bool PCAM = false, bool ROB = false, bool AB = false, bool GEO = false, bool MED = false>
__device__ __forceinline__ void gn_tile(const GnArgs& a, const Pose& pose, const int seq, const int blk, GnTileLds<PPT>& lds,
                                        float* out_row, const Intr& cam, const RobustEntry& rob = RobustEntry{},
                                        const AffineEntry& ab = AffineEntry{}, float* mom_row = nullptr, float (*mred)[8] = nullptr,
                                        const GeoGn& geo = GeoGn{}, unsigned* hist = nullptr);

#if !defined(DVO_GN_WAVES)
#define DVO_GN_WAVES 6   /* waves per SIMD the hot variants are compiled for: 6 = up to 84 VGPRs (78 used, no scratch); at 7 (72 VGPRs) the border sampler spills 24 bytes per lane: 54 MB of extra HBM writes per full-batch launch for the same speed (profiles/r03_patch_sampler_ab.txt) */
#endif
template <int PPT, int G, bool MASK, bool T2D = false>
__global__ void __launch_bounds__(256, (PPT <= 4 && G <= 2) ? DVO_GN_WAVES : 1) k_track_gn(GnArgs a)
{
    __shared__ GnTileLds<PPT> lds;
    // Workgroup 0 clears the counter of the list the following k_gn_solve appends to.  The store comes last on every path:
    // a store ahead of the list / pose loads would make the compiler fetch those through the vector memory path.
    auto clear_next = [&]() {
        if (__builtin_amdgcn_readfirstlane((int)blockIdx.x) == 0 && a.next_count) {  // scalar test first (no VGPR kept for it)
            if (threadIdx.x == 0) *a.next_count = 0;
        }
    };
    // The grid covers the tiles of all sequences, but only those of the ACTIVE ones exist: the workgroups of XCD x
    // (blockIdx % 8 == x) take the x-th contiguous eighth of the n_tiles live tiles (neighbouring tiles share an L2) and
    // every other workgroup leaves after this one scalar load -- converged sequences cost (almost) nothing.
    // Tiles whose rows all lie outside the crop window (optimize.cpp:33-36) are not launched either: only tiles
    // [blk_first, blk_first + blk_count) of a sequence exist, and k_gn_solve reads the others as zero.
    const int n_tiles = (a.list ? a.list[0] : a.n_seq) * a.blk_count;
    const int t8 = (n_tiles + 7) >> 3, xcd = blockIdx.x & 7, tile_in_xcd = (int)(blockIdx.x >> 3);
    const int tile_id = xcd * t8 + tile_in_xcd;
    if (tile_in_xcd >= t8 || tile_id >= n_tiles) {
        clear_next();
        return;
    }
    const int slot = tile_id / a.blk_count, blk = a.blk_first + (tile_id - slot * a.blk_count);
    const int seq = a.list ? a.list[4 + slot] : slot;
    const Pose pose = a.state[seq].pose;              // wave-uniform -> scalar loads
    gn_tile<PPT, G, MASK, T2D>(a, pose, seq, blk, lds, a.partials + ((size_t)seq * a.nblk + blk) * 32, a.k);
    clear_next();
}

// k_track_gn with per-sequence intrinsics (dvo_batch_set_intrinsics, GnArgs::seq_k): line for line k_track_gn, with gn_tile's PCAM
// set.  (A separate kernel rather than a fifth template parameter, and a copy rather than a shared inline body: either of those
// changed the default k_track_gn's instruction schedule.)
template <int PPT, int G, bool MASK, bool T2D = false>
__global__ void __launch_bounds__(256, (PPT <= 4 && G <= 2) ? DVO_GN_WAVES : 1) k_track_gn_cam(GnArgs a)
{
    __shared__ GnTileLds<PPT> lds;
    auto clear_next = [&]() {
        if (__builtin_amdgcn_readfirstlane((int)blockIdx.x) == 0 && a.next_count) {
            if (threadIdx.x == 0) *a.next_count = 0;
        }
    };
    const int n_tiles = (a.list ? a.list[0] : a.n_seq) * a.blk_count;
    const int t8 = (n_tiles + 7) >> 3, xcd = blockIdx.x & 7, tile_in_xcd = (int)(blockIdx.x >> 3);
    const int tile_id = xcd * t8 + tile_in_xcd;
    if (tile_in_xcd >= t8 || tile_id >= n_tiles) {
        clear_next();
        return;
    }
    const int slot = tile_id / a.blk_count, blk = a.blk_first + (tile_id - slot * a.blk_count);
    const int seq = a.list ? a.list[4 + slot] : slot;
    const Pose pose = a.state[seq].pose;
    const Intr cam = a.seq_k[seq];
    gn_tile<PPT, G, MASK, T2D, true>(a, pose, seq, blk, lds, a.partials + ((size_t)seq * a.nblk + blk) * 32, cam);
    clear_next();
}

// track_gn_term_body: the body of every opt-in tile kernel (k_track_gn_rw, _ab, _z and their _cam forms) -- what
// k_track_gn / k_track_gn_cam do (those two stay written out: sharing a body rescheduled them), plus the per-sequence entries of the
// terms that are on, loaded once per workgroup (scalar loads) next to the pose: pose, AffineEntry (AB), RobustEntry (ROB), camera.
// rg / ag / zg and mred are read only under their flag; a kernel passes an empty block (and nullptr) for a term it does not have.
// MED (k_track_gn_md): `hist`, the workgroup's 256 bin counters in LDS, is cleared ahead of the tile, and after it (gn_tile's last
// barrier orders every count) thread t adds a non-zero hist[t] to bin t of the sequence's row of mg.hist.
template <int PPT, int G, bool T2D, bool PCAM, bool ROB, bool AB, bool GEO, bool MED = false>
__device__ __forceinline__ void track_gn_term_body(const GnArgs& a, const RobustGn& rg, const AffineGn& ag, const GeoGn& zg,
                                                   GnTileLds<PPT>& lds, float (*mred)[8], const MedianGn& mg = MedianGn{},
                                                   unsigned* hist = nullptr)
{
    auto clear_next = [&]() {
        if (__builtin_amdgcn_readfirstlane((int)blockIdx.x) == 0 && a.next_count) {
            if (threadIdx.x == 0) *a.next_count = 0;
        }
    };
    const int n_tiles = (a.list ? a.list[0] : a.n_seq) * a.blk_count;
    const int t8 = (n_tiles + 7) >> 3, xcd = blockIdx.x & 7, tile_in_xcd = (int)(blockIdx.x >> 3);
    const int tile_id = xcd * t8 + tile_in_xcd;
    if (tile_in_xcd >= t8 || tile_id >= n_tiles) {
        clear_next();
        return;
    }
    const int slot = tile_id / a.blk_count, blk = a.blk_first + (tile_id - slot * a.blk_count);
    const int seq = a.list ? a.list[4 + slot] : slot;
    const Pose pose = a.state[seq].pose;
    AffineEntry ab{};
    if constexpr (AB) ab = load_seq_entry(ag.table, seq);
    RobustEntry rob{};   // (kind 0 = DVO_ROBUST_NONE: rho = 1)
    if constexpr (ROB) {
        rob = load_seq_entry(rg.table, seq);
        if constexpr (AB) {
            if (ag.prime) rob.kind = DVO_ROBUST_NONE;   // (kernel-uniform: the priming pair is plain)
        }
    }
    Intr cam = a.k;
    if constexpr (PCAM) cam = a.seq_k[seq];
    const size_t row = (size_t)seq * a.nblk + blk;
    float* mom_row = nullptr;
    if constexpr (AB) mom_row = ag.moments + row * 8;
    if constexpr (MED) {
        hist[threadIdx.x] = 0u;
        __syncthreads();
        gn_tile<PPT, G, false, T2D, PCAM, ROB, AB, GEO, true>(a, pose, seq, blk, lds, a.partials + row * 32, cam, rob, ab, mom_row, mred, zg, hist);
        const unsigned n = hist[threadIdx.x];
        if (n != 0u)
            __hip_atomic_fetch_add(mg.hist + (size_t)seq * DVO_MEDIAN_BINS + threadIdx.x, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else
    gn_tile<PPT, G, false, T2D, PCAM, ROB, AB, GEO>(a, pose, seq, blk, lds, a.partials + row * 32, cam, rob, ab, mom_row, mred, zg);
    clear_next();
}

// k_track_gn_rw / k_track_gn_rw_cam: k_track_gn / k_track_gn_cam with robust residual weights (dvo_batch_set_robust_weights, DESIGN.md
// §23): the same tiles, lists, gates and samplers, and the sequence's RobustEntry beside its pose.  Kernels of their own beside the
// plain ones, which stay as they are; no MASK instances (the mask at a pose is the plain kernel's).
#if !defined(DVO_GN_RW_WAVES)
#define DVO_GN_RW_WAVES DVO_GN_WAVES
#endif
template <int PPT, int G, bool T2D = false>
__global__ void __launch_bounds__(256, (PPT <= 4 && G <= 2) ? DVO_GN_RW_WAVES : 1) k_track_gn_rw(GnArgs a, RobustGn rg)
{
    __shared__ GnTileLds<PPT> lds;
    track_gn_term_body<PPT, G, T2D, false, true, false, false>(a, rg, AffineGn{}, GeoGn{}, lds, nullptr);
}
template <int PPT, int G, bool T2D = false>
__global__ void __launch_bounds__(256, (PPT <= 4 && G <= 2) ? DVO_GN_RW_WAVES : 1) k_track_gn_rw_cam(GnArgs a, RobustGn rg)
{
    __shared__ GnTileLds<PPT> lds;
    track_gn_term_body<PPT, G, T2D, true, true, false, false>(a, rg, AffineGn{}, GeoGn{}, lds, nullptr);
}

// k_track_gn_md / k_track_gn_md_cam: k_track_gn_rw / k_track_gn_rw_cam for the median scale (dvo_batch_set_robust_median, DESIGN.md
// §30): the same weighted sums bit for bit, and every contributing pixel's |r| counted in the sequence's 256 bins.  Kernels of their
// own beside the others, which stay as they are.  The LDS add's address and the contributing flag take the hot instances from
// k_track_gn_rw's 78 VGPRs to 81-82, past the 80 that six waves allow (8 to 12 bytes of scratch per lane there): the family is built
// for five waves per SIMD (up to 96 VGPRs), scratch 0.
#if !defined(DVO_GN_MD_WAVES)
#define DVO_GN_MD_WAVES 5
#endif
template <int PPT, int G, bool T2D = false>
__global__ void __launch_bounds__(256, (PPT <= 4 && G <= 2) ? DVO_GN_MD_WAVES : 1) k_track_gn_md(GnArgs a, RobustGn rg, MedianGn mg)
{
    __shared__ GnTileLds<PPT> lds;
    __shared__ unsigned hist[DVO_MEDIAN_BINS];
    track_gn_term_body<PPT, G, T2D, false, true, false, false, true>(a, rg, AffineGn{}, GeoGn{}, lds, nullptr, mg, hist);
}
template <int PPT, int G, bool T2D = false>
__global__ void __launch_bounds__(256, (PPT <= 4 && G <= 2) ? DVO_GN_MD_WAVES : 1) k_track_gn_md_cam(GnArgs a, RobustGn rg, MedianGn mg)
{
    __shared__ GnTileLds<PPT> lds;
    __shared__ unsigned hist[DVO_MEDIAN_BINS];
    track_gn_term_body<PPT, G, T2D, true, true, false, false, true>(a, rg, AffineGn{}, GeoGn{}, lds, nullptr, mg, hist);
}

// k_track_gn_ab / k_track_gn_ab_cam: k_track_gn / k_track_gn_cam (ROB: k_track_gn_rw / k_track_gn_rw_cam) with affine brightness
// compensation (dvo_batch_set_affine_brightness): the same tiles, lists, gates and samplers, and the sequence's
// AffineEntry loaded once per workgroup (scalar loads) next to its pose.  New kernels beside the others, which stay as they are; no
// MASK instances (the mask at a pose is the plain kernel's).
#if !defined(DVO_GN_AB_WAVES)
#define DVO_GN_AB_WAVES 5   /* the hot <4, 1|2, *, *> instances need 81-87 VGPRs for the four or five moment accumulators: at 6 waves (80 allocatable) they spill 8-28 bytes per lane, at 5 there is no scratch */
#endif
// One contributing pixel of k_track_gn_ab, shared by the main loop and the deferred loop: the compensated brightness c, the residual
// against it, and the pixel's brightness moments M = (M0, M1, M2, M11, M12) with p = rho * I1 (one rounded multiply).  A rejected
// pixel (ok = false) adds exact zeros; without ROB rho is 1 and M0 is not kept (the solve uses n_valid).
template <bool ROB>
__device__ __forceinline__ void affine_pixel(const AffineEntry& ab, const RobustEntry& rob, const bool ok, const float wgt, const float I1,
                                             const float I2, float& r, float& rw, float& rho, float (&M)[DVO_AFFINE_MOMENTS])
{
    const float c = fmaf(ab.a, I1, ab.b);
    r = ok ? I2 - c : 0.0f;
    rw = ok ? r * wgt : 0.0f;
    const float i1 = ok ? I1 : 0.0f, i2 = ok ? I2 : 0.0f;
    if constexpr (ROB) {
        rho = ok ? robust_rho(rob, r) : 1.0f;   // (never used for a rejected pixel: 1 keeps a non-finite quotient out of the sums)
        const float rz = ok ? rho : 0.0f;
        const float p = rz * i1;
        M[0] += rz;
        M[1] += p;
        M[2] = fmaf(rz, i2, M[2]);
        M[3] = fmaf(p, i1, M[3]);
        M[4] = fmaf(p, i2, M[4]);
    } else {   // rho = 1: p = I1 and fmaf(1, I2, M2) = M2 + I2, the same bits
        rho = 1.0f;
        M[1] += i1;
        M[2] += i2;
        M[3] = fmaf(i1, i1, M[3]);
        M[4] = fmaf(i1, i2, M[4]);
    }
}
template <int PPT, int G, bool T2D = false, bool ROB = false>
__global__ void __launch_bounds__(256, (PPT <= 4 && G <= 2) ? DVO_GN_AB_WAVES : 1) k_track_gn_ab(GnArgs a, RobustGn rg, AffineGn ag)
{
    __shared__ GnTileLds<PPT> lds;
    __shared__ float mred[4][8];
    track_gn_term_body<PPT, G, T2D, false, ROB, true, false>(a, rg, ag, GeoGn{}, lds, mred);
}
template <int PPT, int G, bool T2D = false, bool ROB = false>
__global__ void __launch_bounds__(256, (PPT <= 4 && G <= 2) ? DVO_GN_AB_WAVES : 1) k_track_gn_ab_cam(GnArgs a, RobustGn rg, AffineGn ag)
{
    __shared__ GnTileLds<PPT> lds;
    __shared__ float mred[4][8];
    track_gn_term_body<PPT, G, T2D, true, ROB, true, false>(a, rg, ag, GeoGn{}, lds, mred);
}

// k_track_gn_z / k_track_gn_z_cam: k_track_gn / k_track_gn_cam with the geometric (depth) term of a sensor-depth batch
// (dvo_batch_set_geometric): the same tiles, lists, gates and samplers on the tracked frame's own depth and weight,
// plus twelve reference-depth taps per fast-path pixel.  New kernels beside the others, which stay as they are; no MASK instances.
#if !defined(DVO_GN_Z_WAVES)
#define DVO_GN_Z_WAVES 3   /* the hot <4, 1|2, *> instances keep 12 more taps per pixel in flight and two more accumulators: 133-144 VGPRs, no scratch at 3 waves (168 allocatable); at 4 waves (128) they spill 8-48 bytes per lane, at 5 (96) 128-172, at 6 (80) 196-228 */
#endif
__device__ __forceinline__ float max3_raw(float a, float b, float c)   // (min3_raw's counterpart)
{
    float m;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(m) : "v"(a), "v"(b), "v"(c));
    return m;
}
// The geometric row of one fast-path pixel (include/dvo.h, dvo_batch_set_geometric).  ok: the pixel contributes its photometric row;
// t: the 12 reference-depth taps of its footprint; Zw: the transformed point's z.  A pixel without a geometric row has its operands
// selected to zero first and adds exact zeros, so a NaN or inf tap never reaches a sum.
__device__ __forceinline__ void geo_pixel(const Intr& k, const GeoGn& geo, const float min_depth, const bool ok, const int x, const int y,
                                          const float d, const float iz, const float wgt, const Taps& t, const float u, const float v,
                                          const int x0, const int y0, const float Zw, Acc29& acc, float& S29, float& S30)
{
    const float hx = u - (float)x0, vy = v - (float)y0;
    const float Zs = blend4(t.rb.y, t.rb.z, t.rc.y, t.rc.z, hx, vy);
    const float gzx = blend4(t.rb.z - t.rb.x, t.rb.w - t.rb.y, t.rc.z - t.rc.x, t.rc.w - t.rc.y, hx, vy);
    const float gzy = blend4(t.rc.y - t.ra.x, t.rc.z - t.ra.y, t.rd.x - t.rb.y, t.rd.y - t.rb.z, hx, vy);
    // all 12 taps finite and >= min_depth: the smallest and the largest tap, and a probe that a NaN or inf tap poisons (0 * inf = NaN)
    const float mn = min3_raw(min3_raw(min3_raw(t.ra.x, t.ra.y, t.rd.x), min3_raw(t.rb.x, t.rb.y, t.rb.z), min3_raw(t.rc.x, t.rc.y, t.rc.z)),
                              min3_raw(t.rd.y, t.rb.w, t.rc.w), t.rd.y);
    const float mx = max3_raw(max3_raw(max3_raw(t.ra.x, t.ra.y, t.rd.x), max3_raw(t.rb.x, t.rb.y, t.rb.z), max3_raw(t.rc.x, t.rc.y, t.rc.z)),
                              max3_raw(t.rd.y, t.rb.w, t.rc.w), t.rd.y);
    const float probe = (Zs + gzx) + gzy;
    const float rz = Zs - Zw;
    const bool on = ok & (mn >= min_depth) & (mx < __builtin_inff()) & (probe == probe) & (fabsf(rz) <= geo.max_diff);   // false for NaN
    float Jz[6], r_, rw_;
    gn_jacobian_pre(k, x, y, d, iz, wgt, gzx, gzy, 0.0f, 0.0f, Jz, r_, rw_);
    float X, Y, Z;
    back_project(k, (float)x, (float)y, d, X, Y, Z);
    Jz[2] = Jz[2] - 1.0f;
    Jz[3] = Jz[3] - Y;
    Jz[4] = Jz[4] + X;
    const float lam = geo.weight * (iz * iz);
    float Jg[6];
#pragma unroll
    for (int q = 0; q < 6; q++) Jg[q] = on ? lam * Jz[q] : 0.0f;
    const float rg = on ? lam * rz : 0.0f;
    const float rgw = on ? rg * wgt : 0.0f;
    int idx = 0;
#pragma unroll
    for (int p = 0; p < 6; p++)
#pragma unroll
        for (int q = p; q < 6; q++) {
            acc.a[idx] = fmaf(Jg[p], Jg[q], acc.a[idx]);
            idx++;
        }
#pragma unroll
    for (int p = 0; p < 6; p++) acc.a[21 + p] = fmaf(Jg[p], rgw, acc.a[21 + p]);
    S29 = fmaf(rg, rg, S29);
    S30 += on ? 1.0f : 0.0f;
}
template <int PPT, int G, bool T2D = false>
__global__ void __launch_bounds__(256, (PPT <= 4 && G <= 2) ? DVO_GN_Z_WAVES : 1) k_track_gn_z(GnArgs a, GeoGn zg)
{
    __shared__ GnTileLds<PPT> lds;
    __shared__ float mred[4][8];
    track_gn_term_body<PPT, G, T2D, false, false, false, true>(a, RobustGn{}, AffineGn{}, zg, lds, mred);
}
template <int PPT, int G, bool T2D = false>
__global__ void __launch_bounds__(256, (PPT <= 4 && G <= 2) ? DVO_GN_Z_WAVES : 1) k_track_gn_z_cam(GnArgs a, GeoGn zg)
{
    __shared__ GnTileLds<PPT> lds;
    __shared__ float mred[4][8];
    track_gn_term_body<PPT, G, T2D, true, false, false, true>(a, RobustGn{}, AffineGn{}, zg, lds, mred);
}

// k_track_gn_zab / k_track_gn_zab_cam: k_track_gn_z / k_track_gn_z_cam with affine brightness compensation on the photometric row
// (dvo_batch_set_geometric_affine): the body with both flags.  The geometric row does not see the AffineEntry; the
// moments are k_track_gn_ab's without robust weights.  New kernels beside the others, which stay as they are; no MASK instances.
#if !defined(DVO_GN_ZAB_WAVES)
#define DVO_GN_ZAB_WAVES 3   /* the hot <4, 1|2, *> instances: k_track_gn_z's registers and four moment accumulators, no scratch at 3 waves (168 allocatable) */
#endif
template <int PPT, int G, bool T2D = false>
__global__ void __launch_bounds__(256, (PPT <= 4 && G <= 2) ? DVO_GN_ZAB_WAVES : 1) k_track_gn_zab(GnArgs a, AffineGn ag, GeoGn zg)
{
    __shared__ GnTileLds<PPT> lds;
    __shared__ float mred[4][8];
    track_gn_term_body<PPT, G, T2D, false, false, true, true>(a, RobustGn{}, ag, zg, lds, mred);
}
template <int PPT, int G, bool T2D = false>
__global__ void __launch_bounds__(256, (PPT <= 4 && G <= 2) ? DVO_GN_ZAB_WAVES : 1) k_track_gn_zab_cam(GnArgs a, AffineGn ag, GeoGn zg)
{
    __shared__ GnTileLds<PPT> lds;
    __shared__ float mred[4][8];
    track_gn_term_body<PPT, G, T2D, true, false, true, true>(a, RobustGn{}, ag, zg, lds, mred);
}

// One contributing pixel into the workgroup's bin counters (k_track_gn_md): one LDS integer add without a return value per
// contributing lane.  A tile's residuals crowd into a few bins, so lanes of a wave meet at one LDS address; the hardware's
// serialisation of those costs +15 % per finest-level launch against k_track_gn_rw.  DVO_MD_AGGREGATE = 1 is the form that was
// measured against it: per wave one add of the population count per distinct bin among its contributing lanes (rounds of ballot +
// readlane, all scalar).  It keeps 78 VGPRs and six waves, but its rounds cost 3.8 times k_track_gn_rw's launch.
// Integer sums: any order.
#if !defined(DVO_MD_AGGREGATE)
#define DVO_MD_AGGREGATE 0
#endif
__device__ __forceinline__ void median_count(unsigned* hist, const bool ok, const float r)
{
    const int bin = median_bin(r);
#if DVO_MD_AGGREGATE
    unsigned long long todo = __ballot(ok);
    while (todo != 0ull) {   // wave-uniform: one round per distinct bin among the contributing lanes
        const int leader = __builtin_ctzll(todo);
        const int b = __builtin_amdgcn_readlane(bin, leader);
        const unsigned long long same = __ballot(ok && bin == b);
        if ((int)(threadIdx.x & 63) == leader) __hip_atomic_fetch_add(&hist[b], (unsigned)__popcll(same), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        todo &= ~same;
    }
#else
    if (ok) __hip_atomic_fetch_add(&hist[bin], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#endif
}

template <int PPT, int G, bool MASK, bool T2D, bool PCAM, bool ROB, bool AB, bool GEO, bool MED>
__device__ __forceinline__ void gn_tile(const GnArgs& a, const Pose& pose, const int seq, const int blk, GnTileLds<PPT>& lds,
                                        float* out_row, const Intr& cam, const RobustEntry& rob, const AffineEntry& ab, float* mom_row,
                                        float (*mred)[8], const GeoGn& geo, unsigned* hist)
{
    static_assert(!MED || (ROB && !AB && !GEO), "the median scale bins the residual of the robust weights alone");
    float (&red)[4][32] = lds.red;
    int (&slow_q)[4][PPT * 64] = lds.slow_q;
    int (&slow_cnt)[4] = lds.slow_cnt;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // wave-uniform: lives in an SGPR
    const int w = a.w, h = a.h, npix = w * h;
    int nslow = 0;                                    // wave-uniform
    const size_t img_off = (size_t)seq * a.w * a.h;
    const float* __restrict__ obj = a.obj_gray + img_off;
    const float* __restrict__ dep = a.ref_depth + img_off;
    const float* __restrict__ wgp = a.ref_wgt ? a.ref_wgt + img_off : nullptr;   // nullptr: one weight for every contributing pixel
    const float* __restrict__ refp = a.ref_gray + img_off;
    const float wlim = (float)(w - 2), hlim = (float)(h - 2);

    Acc29 acc;
    acc.zero();
    float M[DVO_AFFINE_MOMENTS] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};   // AB: the thread's brightness moments (affine_pixel)
    float S29 = 0.0f, S30 = 0.0f;                                    // GEO: sum rg^2 and n_geo of the thread (geo_pixel)
    // G pixels per thread have their gathers in flight together (memory-level parallelism hides the L2/HBM latency)
    static_assert(PPT % G == 0, "PPT must be a multiple of G");
    // pixel k of this thread: coordinates (xA, yA), linear index iA (clamped into the image), inA = it exists
    int xA[PPT], yA[PPT], iA[PPT];
    bool inA[PPT];
    if constexpr (T2D) {  // GnTiling (dvo_kernels.h): TW = 2^t_shift columns, 64 / TW rows per wave-load
        const int sh = a.t_shift, rw = 64 >> sh;
        const int ty = blk / a.tiles_x, tx = blk - ty * a.tiles_x;
        const int x = a.x_org + (tx << sh) + (lane & ((1 << sh) - 1));
        const int y0 = a.y_org + (ty * (4 * PPT) + wave * PPT) * rw + (lane >> sh);
        const int xc = x < w ? x : w - 1;
#pragma unroll
        for (int k = 0; k < PPT; k++) {
            xA[k] = x; yA[k] = y0 + k * rw;
            inA[k] = (x < w) & (yA[k] < h);
            iA[k] = (int)__umul24((unsigned)(yA[k] < h ? yA[k] : h - 1), (unsigned)w) + xc;
        }
    } else {
        const int base = blk * (256 * PPT) + threadIdx.x;
        // (x, y) of this thread's first pixel by one index split; every further pixel is 256 later in raster order
        split_index(base < npix ? base : npix - 1, w, a.inv_w, xA[0], yA[0]);
#pragma unroll
        for (int k = 1; k < PPT; k++) {
            const int xn = xA[k - 1] + a.r256;
            const int wrap = xn >= w ? 1 : 0;
            xA[k] = xn - wrap * w;
            yA[k] = yA[k - 1] + a.q256 + wrap;
        }
#pragma unroll
        for (int k = 0; k < PPT; k++) {
            const int i = base + k * 256;
            inA[k] = i < npix;  // (coordinates past the end of the image are garbage: gated out)
            iA[k] = inA[k] ? i : npix - 1;
        }
    }
    // every coalesced row load of this thread's PPT pixels is issued up front (independent of the pose): one exposed
    // memory round trip per wave instead of one per group
    float dA[PPT], I1A[PPT], wgA[PPT];
#pragma unroll
    for (int k = 0; k < PPT; k++) {  // ref_depth, obj_gray, weight
        const unsigned ic = (unsigned)iA[k] * 4u;  // byte offset: SGPR base + 32-bit VGPR offset
        dA[k] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(dep) + ic);
        I1A[k] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(obj) + ic);
        wgA[k] = a.wgt_const;
        if (wgp) wgA[k] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(wgp) + ic);   // (wave-uniform)
    }
#pragma unroll
    for (int g0 = 0; g0 < PPT; g0 += G) {
        float d[G], I1[G], iz[G], wg[G], u[G], v[G];
        int xs[G], ys[G], x0[G], y0[G];
        bool gate[G], inter[G];
        Taps t[G];
        Taps tz[GEO ? G : 1];   // GEO: the reference-depth taps of the same footprints
        float Zw[GEO ? G : 1];  // GEO: the transformed point's z
#pragma unroll
        for (int k = 0; k < G; k++) {
            d[k] = dA[g0 + k]; I1[k] = I1A[g0 + k]; wg[k] = wgA[g0 + k];
        }
#pragma unroll
        for (int k = 0; k < G; k++) {  // gates, warp, issue the gathers (always from a safe address)
            xs[k] = xA[g0 + k]; ys[k] = yA[g0 + k];
            // gn_gate (optimize.cpp:33-48) written with bitwise ops so it stays a predicate, not a branch
            bool crop_ok = true;
            if (a.prm.crop) crop_ok = (xs[k] >= 20) & (xs[k] <= 140) & (ys[k] >= 20) & (ys[k] <= 100);  // wave-uniform branch
            gate[k] = inA[g0 + k] & crop_ok & !(d[k] < a.prm.min_depth) & !is_invalid(I1[k]);
            iz[k] = recip_gated(d[k], gate[k]);   // 1.0f / depth (optimize.cpp:70-74) of the pixels that can contribute
            if constexpr (GEO) {   // warp()'s three operations, keeping the z they form
                float X, Y, Z, Xw, Yw;
                back_project(seq_intr<PCAM>(a, cam), (float)xs[k], (float)ys[k], d[k], X, Y, Z);
                transform(pose, X, Y, Z, Xw, Yw, Zw[k]);
                project(seq_intr<PCAM>(a, cam), Xw, Yw, Zw[k], u[k], v[k]);
            } else
            warp(pose, seq_intr<PCAM>(a, cam), (float)xs[k], (float)ys[k], d[k], u[k], v[k]);
            inter[k] = gate[k] & (u[k] >= 1.0f) & (v[k] >= 1.0f) & (u[k] < wlim) & (v[k] < hlim);  // false for NaN
            x0[k] = inter[k] ? (int)u[k] : 1;
            y0[k] = inter[k] ? (int)v[k] : 1;
            // unsigned 32-bit element offsets from the wave-uniform base: SGPR-base + VGPR-offset addressing, no 64-bit VALU math
            // (24-bit multiply: full rate, v_mul_lo_u32 is quarter rate; y0 < h and w are far below 2^24)
            const unsigned c = (__umul24((unsigned)y0[k], (unsigned)w) + (unsigned)x0[k]) * 4u, uw = (unsigned)w * 4u;  // BYTE offsets (< 2^26)
            const char* rb8 = reinterpret_cast<const char*>(refp);
            t[k].ra = *reinterpret_cast<const f2u*>(rb8 + (c - uw));
            t[k].rb = *reinterpret_cast<const f4u*>(rb8 + (c - 4u));
            t[k].rc = *reinterpret_cast<const f4u*>(rb8 + (c + uw - 4u));
            t[k].rd = *reinterpret_cast<const f2u*>(rb8 + (c + 2u * uw));
            if constexpr (GEO) {   // the same byte offsets into the reference depth: in flight with the gray taps
                const char* zb8 = reinterpret_cast<const char*>(geo.ref_z + img_off);
                tz[k].ra = *reinterpret_cast<const f2u*>(zb8 + (c - uw));
                tz[k].rb = *reinterpret_cast<const f4u*>(zb8 + (c - 4u));
                tz[k].rc = *reinterpret_cast<const f4u*>(zb8 + (c + uw - 4u));
                tz[k].rd = *reinterpret_cast<const f2u*>(zb8 + (c + 2u * uw));
            }
        }
        // The G pixels are sampled in ONE straight-line block (independent chains interleave: ILP), the rare generic
        // sampler runs in a single separate region, then Jacobians and sums again in one straight-line block.
        float I2[G], gx[G], gy[G];
        bool okf[G];
#pragma unroll
        for (int k = 0; k < G; k++) {
            bool decidable, valid;
            gn_sample_fast(t[k], u[k], v[k], x0[k], y0[k], I2[k], gx[k], gy[k], decidable, valid);
            const bool fast = inter[k] & decidable;  // (inter implies gate)
            okf[k] = fast & valid;
            // Everything else that passed the gate -- the band along the border, positions outside the image (rejected by
            // optimize.cpp:52-56), INVALID or NaN taps -- is left to the generic sampler.  A few lanes per wave need it, so
            // running it here would cost the whole wave ~350 instructions and several dependent round trips per occurrence;
            // instead the pixel index is queued (per wave, lane order: deterministic) and the workgroup evaluates all of
            // its deferred pixels densely after the main loop.
            const bool cand = gate[k] & !fast;
            if (__ballot(cand) == 0ull) continue;  // wave-uniform; the common case in the interior of the image
            // (a position outside [0,w) x [0,h), or NaN, is rejected by optimize.cpp:52-56 whatever the samplers say)
            const bool inside = (u[k] >= 0.0f) & (v[k] >= 0.0f) & (u[k] < (float)w) & (v[k] < (float)h);
            const bool slow = cand & inside;
            const unsigned long long bal = __ballot(slow);
            if (bal != 0ull) {  // wave-uniform
                if (slow) {
                    const int pos = nslow + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
                    slow_q[wave][pos] = (int)__umul24((unsigned)ys[k], (unsigned)w) + xs[k];  // (recomputed: iA is dead after the loads)
                }
                nslow += __popcll(bal);
            }
        }
#pragma unroll
        for (int k = 0; k < G; k++) {
            // predicated accumulation: rejected pixels add exact zeros, so no control flow merges the 29 accumulators
            const bool ok = okf[k];
            float J[6], r, rw;
            gn_jacobian_pre(seq_intr<PCAM>(a, cam), xs[k], ys[k], d[k], iz[k], wg[k], gx[k], gy[k], I1[k], I2[k], J, r, rw);
#pragma unroll
            for (int q = 0; q < 6; q++) J[q] = ok ? J[q] : 0.0f;
            if constexpr (AB) {
                float rho;
                affine_pixel<ROB>(ab, rob, ok, wg[k], I1[k], I2[k], r, rw, rho, M);
                if constexpr (ROB) acc.add_w(J, r, rw, ok ? 1.0f : 0.0f, rho);
                else acc.add(J, r, rw, ok ? 1.0f : 0.0f);
            } else
            if constexpr (ROB) {   // (a rejected pixel's rho is never used: its row is zeros, and 1 keeps a non-finite quotient out of the sums)
                const float rs = ok ? r : 0.0f;
                acc.add_w(J, rs, ok ? rw : 0.0f, ok ? 1.0f : 0.0f, ok ? robust_rho(rob, rs) : 1.0f);
                if constexpr (MED) median_count(hist, ok, rs);
            } else
            acc.add(J, ok ? r : 0.0f, ok ? rw : 0.0f, ok ? 1.0f : 0.0f);
            if constexpr (GEO)   // after the pixel's photometric add (ok implies the fast path: interior footprint, 12 valid gray taps)
                geo_pixel(seq_intr<PCAM>(a, cam), geo, a.prm.min_depth, ok, xs[k], ys[k], d[k], iz[k], wg[k], tz[k], u[k], v[k], x0[k], y0[k],
                          Zw[k], acc, S29, S30);
            if (MASK && ok) a.mask[img_off + (size_t)(ys[k] * w + xs[k])] = 1;
        }
    }
    // deferred pixels: the four wave queues, concatenated in wave order, are spread densely over the workgroup's threads
    if (lane == 0) slow_cnt[wave] = nslow;
    __syncthreads();
    {
        const int c0 = slow_cnt[0], c1 = c0 + slow_cnt[1], c2 = c1 + slow_cnt[2], total = c2 + slow_cnt[3];
        for (int e = threadIdx.x; e < total; e += 256) {
            const int qw = (e >= c0) + (e >= c1) + (e >= c2);
            const int qoff = qw == 0 ? 0 : (qw == 1 ? c0 : (qw == 2 ? c1 : c2));
            const int i = slow_q[qw][e - qoff];  // < npix (only gated pixels are queued)
            int x, y;
            split_index(i, w, a.inv_w, x, y);
            // (carrying d and I1 through LDS with the index instead of re-loading them: measured in the LAT form, no change)
            const float d = dep[i], I1 = obj[i], iz = recip_gated(dep[i], true), wg = wgp ? wgp[i] : a.wgt_const;
            float u, v;
            warp(pose, seq_intr<PCAM>(a, cam), (float)x, (float)y, d, u, v);  // same operations on the same inputs as in the main loop
            // inlined (single site): a call here would pin the 29 live accumulators to callee-saved registers and
            // raise the kernel's VGPR allocation.  (Tried: the sampler on a register patch of 12 taps loaded up front from
            // clamped coordinates -- one round trip, no divergent loads.  Slower by 20 % on the probe: the branches of the
            // memory version skip most of the work for most border pixels.)
            SlowSample ss;
            ss.ok = gn_sample_patch(refp, w, h, d, u, v, ss.I2, ss.gx, ss.gy) ? 1 : 0;
            const bool ok = ss.ok != 0;
            float J[6], r, rw;
            gn_jacobian_pre(seq_intr<PCAM>(a, cam), x, y, d, iz, wg, ss.gx, ss.gy, I1, ss.I2, J, r, rw);
#pragma unroll
            for (int q = 0; q < 6; q++) J[q] = ok ? J[q] : 0.0f;
            if constexpr (AB) {   // the same operations as in the main loop
                float rho;
                affine_pixel<ROB>(ab, rob, ok, wg, I1, ss.I2, r, rw, rho, M);
                if constexpr (ROB) acc.add_w(J, r, rw, ok ? 1.0f : 0.0f, rho);
                else acc.add(J, r, rw, ok ? 1.0f : 0.0f);
            } else
            if constexpr (ROB) {   // the same operations as in the main loop
                const float rs = ok ? r : 0.0f;
                acc.add_w(J, rs, ok ? rw : 0.0f, ok ? 1.0f : 0.0f, ok ? robust_rho(rob, rs) : 1.0f);
                if constexpr (MED) median_count(hist, ok, rs);
            } else
            acc.add(J, ok ? r : 0.0f, ok ? rw : 0.0f, ok ? 1.0f : 0.0f);
            if (MASK && ok) a.mask[img_off + i] = 1;
        }
    }
    // wave reduction (DPP), then 4 waves through LDS in fixed order
    {
        float o0, o1;
        wave_reduce29_packed(acc.a, o0, o1);
        if ((lane & 3) == 0) {  // one lane per quad publishes its value (slots 29..31 are zero padding)
            red[wave][packed_slot_index(lane, 0)] = o0;
            red[wave][packed_slot_index(lane, 1)] = o1;
        }
    }
    if constexpr (AB) {   // the moments: a six-step butterfly per wave (every lane ends with the same bits), lane 0 publishes
#pragma unroll
        for (int m = ROB ? 0 : 1; m < DVO_AFFINE_MOMENTS; m++) {
            float v = M[m];
            v += __shfl_xor(v, 32); v += __shfl_xor(v, 16); v += __shfl_xor(v, 8);
            v += __shfl_xor(v, 4); v += __shfl_xor(v, 2); v += __shfl_xor(v, 1);
            if (lane == 0) mred[wave][m] = v;
        }
        if (lane == 0 && !ROB) mred[wave][0] = 0.0f;
    }
    // GEO: where a wave hands over its slots 29 and 30 in mred: beside the five moments when both terms are on (k_track_gn_zab), which
    // publish mred[wave][0..4] ahead of the same barrier
    constexpr int ZR = (AB && GEO) ? DVO_AFFINE_MOMENTS : 0;
    if constexpr (GEO) {   // slots 29 and 30: the moments' butterfly (every lane ends with the same bits), lane 0 publishes
        float v29 = S29, v30 = S30;
        v29 += __shfl_xor(v29, 32); v29 += __shfl_xor(v29, 16); v29 += __shfl_xor(v29, 8);
        v29 += __shfl_xor(v29, 4); v29 += __shfl_xor(v29, 2); v29 += __shfl_xor(v29, 1);
        v30 += __shfl_xor(v30, 32); v30 += __shfl_xor(v30, 16); v30 += __shfl_xor(v30, 8);
        v30 += __shfl_xor(v30, 4); v30 += __shfl_xor(v30, 2); v30 += __shfl_xor(v30, 1);
        if (lane == 0) { mred[wave][ZR] = v29; mred[wave][ZR + 1] = v30; }
    }
    __syncthreads();
    if (threadIdx.x < 32) {
        const int c = threadIdx.x;
        float s = 0.0f;
        if (c < 29) s = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
        if constexpr (GEO) {   // the four waves in wave order, into the row's free slots
            if (c == 29 || c == 30) s = ((mred[0][c - 29 + ZR] + mred[1][c - 29 + ZR]) + mred[2][c - 29 + ZR]) + mred[3][c - 29 + ZR];
        }
        out_row[c] = s;
    }
    if constexpr (AB) {   // the four waves in wave order, as above (wave 1 stores: the two rows go out side by side)
        if (threadIdx.x >= 64 && threadIdx.x < 72) {
            const int c = threadIdx.x - 64;
            float s = 0.0f;
            if (c < DVO_AFFINE_MOMENTS) s = ((mred[0][c] + mred[1][c]) + mred[2][c]) + mred[3][c];
            mom_row[c] = s;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// k_track_gn_tile: same arithmetic as k_track_gn, different data movement.  A workgroup owns a 64 x (4*PPT)
// pixel tile; it first issues ALL of its global loads in one burst -- the coalesced rows of its own pixels and
// the reference-gray patch (tile grown by `margin` pixels plus the 4x4 tap footprint) into LDS -- then, after one
// barrier, every warped sample is a short-latency LDS read instead of an L1/L2 gather.  Pixels whose footprint
// leaves the staged patch (large motion) gather from global memory; borders / INVALID taps take the generic
// sampler.  All three sources hold the same floats, so results are bit-identical.
// ------------------------------------------------------------------------------------------------
template <int PPT, bool MASK, bool PCAM>   // PCAM: per-sequence intrinsics (seq_intr)
__global__ void __launch_bounds__(256) k_track_gn_tile(GnArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];  // [0,128): reduction scratch, then the patch
    float* red = smem;
    float* patch = smem + 128;
    const unsigned id = xcd_remap(blockIdx.x, gridDim.x);
    const int seq = id / a.nblk, tile = id - seq * a.nblk;
    const SeqState& st = a.state[seq];
    if (!a.ignore_active && st.active == 0) return;  // converged sequences cost nothing
    if (a.plan_action && a.plan_action[seq] != DVO_SEQ_TRACK) return;   // not tracked by this push (Batch plan): ignore_active does not enable it
    const Pose pose = st.pose;
    Intr cam;
    if constexpr (PCAM) cam = a.seq_k[seq];   // (before the patch stores and the barrier: scalar loads)
    const int w = a.w, h = a.h;
    constexpr int TH = 4 * PPT;
    const int tyi = tile / a.tiles_x, txi = tile - tyi * a.tiles_x;
    const int tx0 = txi * 64, ty0 = tyi * TH;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t img_off = (size_t)seq * w * h;
    const float* __restrict__ obj = a.obj_gray + img_off;
    const float* __restrict__ dep = a.ref_depth + img_off;
    const float* __restrict__ wgp = a.ref_wgt ? a.ref_wgt + img_off : nullptr;
    const float* __restrict__ refp = a.ref_gray + img_off;

    // ---- one burst of global loads: own pixels (registers) + reference patch (LDS) ----
    const int x = tx0 + lane;
    float d[PPT], I1[PPT], iz[PPT], wg[PPT];
#pragma unroll
    for (int k = 0; k < PPT; k++) {
        const int y = ty0 + wave + 4 * k;
        const int xc = x < w ? x : w - 1, yc = y < h ? y : h - 1;  // clamped: no branch, gated out below
        const int i = yc * w + xc;
        d[k] = dep[i];
        I1[k] = obj[i];
        iz[k] = 0.0f;
        wg[k] = wgp ? wgp[i] : a.wgt_const;
    }
    const int M = a.margin, PW = 64 + 2 * M + 3;
    const int px0 = max(tx0 - M - 1, 0), px1 = min(tx0 + 64 + M + 2, w);  // staged columns [px0, px1)
    const int py0 = max(ty0 - M - 1, 0), py1 = min(ty0 + TH + M + 2, h);  // staged rows    [py0, py1)
    for (int r = py0 + wave; r < py1; r += 4) {
        const float* src = refp + r * w;
        float* dst = patch + (r - py0) * PW;
        for (int c = px0 + lane; c < px1; c += 64) dst[c - px0] = src[c];
    }
    __syncthreads();

    const float wlim = (float)(w - 2), hlim = (float)(h - 2);
    Acc29 acc;
    acc.zero();
#pragma unroll
    for (int k = 0; k < PPT; k++) {
        const int y = ty0 + wave + 4 * k;
        const int crop_ok = (a.prm.crop == 0) | ((x >= 20) & (x <= 140) & (y >= 20) & (y <= 100));
        const bool gate = (x < w) & (y < h) & (crop_ok != 0) & !(d[k] < a.prm.min_depth) & !is_invalid(I1[k]);
        iz[k] = recip_gated(d[k], gate);
        float u, v;
        warp(pose, seq_intr<PCAM>(a, cam), (float)x, (float)y, d[k], u, v);
        const bool inter = gate & (u >= 1.0f) & (v >= 1.0f) & (u < wlim) & (v < hlim);  // false for NaN
        const int x0 = inter ? (int)u : 1, y0 = inter ? (int)v : 1;
        const bool inpatch = inter & (x0 - 1 >= px0) & (x0 + 2 < px1) & (y0 - 1 >= py0) & (y0 + 2 < py1);
        Taps t;
        {  // LDS taps (address forced inside the patch for lanes that will not use them)
            const int lx = inpatch ? x0 - px0 : 1, ly = inpatch ? y0 - py0 : 1;
            const float* q = patch + ly * PW + lx;
            t.ra.x = q[-PW]; t.ra.y = q[-PW + 1];
            t.rb.x = q[-1]; t.rb.y = q[0]; t.rb.z = q[1]; t.rb.w = q[2];
            t.rc.x = q[PW - 1]; t.rc.y = q[PW]; t.rc.z = q[PW + 1]; t.rc.w = q[PW + 2];
            t.rd.x = q[2 * PW]; t.rd.y = q[2 * PW + 1];
        }
        if (inter & !inpatch) {  // footprint left the staged patch (large motion): gather from global memory
            const float* p = refp + (y0 * w + x0);
            t.ra = *reinterpret_cast<const f2u*>(p - w);
            t.rb = *reinterpret_cast<const f4u*>(p - 1);
            t.rc = *reinterpret_cast<const f4u*>(p + w - 1);
            t.rd = *reinterpret_cast<const f2u*>(p + 2 * w);
        }
        float I2 = 0.0f, gx = 0.0f, gy = 0.0f;
        bool decidable, valid;
        gn_sample_fast(t, u, v, x0, y0, I2, gx, gy, decidable, valid);
        int s = decidable ? (valid ? 1 : 0) : -1;
        const bool inside = (u >= 0.0f) & (v >= 0.0f) & (u < (float)w) & (v < (float)h);  // outside: rejected (optimize.cpp:52-56)
        s = (gate & inside) ? (inter ? s : -1) : 0;
        if (s < 0) {  // border, INVALID or NaN taps: the generic sampler decides (rare; a real function call)
            const SlowSample ss = gn_sample_slow(refp, w, h, d[k], u, v);
            s = ss.ok; I2 = ss.I2; gx = ss.gx; gy = ss.gy;
        }
        const bool ok = s > 0;
        float J[6], r, rw;
        gn_jacobian_pre(seq_intr<PCAM>(a, cam), x, y, d[k], iz[k], wg[k], gx, gy, I1[k], I2, J, r, rw);
#pragma unroll
        for (int q = 0; q < 6; q++) J[q] = ok ? J[q] : 0.0f;
        acc.add(J, ok ? r : 0.0f, ok ? rw : 0.0f, ok ? 1.0f : 0.0f);
        if (MASK && ok) a.mask[img_off + y * w + x] = 1;
    }
    // wave reduction (DPP, step-major), then the 4 waves through LDS in fixed order
    {
        float o0, o1;
        wave_reduce29_packed(acc.a, o0, o1);
        if ((lane & 3) == 0) {
            red[wave * 32 + packed_slot_index(lane, 0)] = o0;
            red[wave * 32 + packed_slot_index(lane, 1)] = o1;
        }
    }
    __syncthreads();
    if (threadIdx.x < 32) {
        const int c = threadIdx.x;
        float s = 0.0f;
        if (c < 29) s = ((red[c] + red[32 + c]) + red[64 + c]) + red[96 + c];
        a.partials[((size_t)seq * a.nblk + tile) * 32 + c] = s;
    }
}

// ------------------------------------------------------------------------------------------------
// k_gn_solve: second reduction stage + the rest of one Tracker::track iteration (tracker.cpp:44-73),
// one 64-thread workgroup per sequence, entirely on the device:
//   partial sums -> double, fixed order;  xi_update = H^+ g (LDL^T / eigen pseudo-inverse, double);
//   xi <- log(exp(xi) exp(xi_update)) unless NaN (testXi);  pose <- exp(-xi);  stop tests.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int solve_finish(const SolveArgs& a, const int seq, SeqState& st, const double* tot, const int first,
                                            const int it_prev, float xi[6], double Tc[12], Pose& np);

// DVO_SOLVE_SEQ sequences per 256-thread workgroup.  The serial chain below (6x6 solve, exp / log in double: ~4.4 us,
// ~250 VGPRs) is the same instruction stream for every sequence, so lanes 0..7 of wave 0 run it for 8 sequences in lockstep
// at the price of one; with one sequence per workgroup a 4096-sequence batch needed several rounds of workgroups, each
// waiting out a full chain.  Stage one: team t (32 lanes = the 32 columns of a partial row) sums the rows of sequence t.
#define DVO_SOLVE_SEQ 8
#define DVO_SOLVE_GROUPS 4   /* row classes of the fixed summation order: rows b = g (mod 4) in batches of 8, then (s0+s1)+(s2+s3) */
// Second reduction stage for one column of one sequence: the workgroup partials p[b * 32], b = 0 .. nblk-1, summed in double in a
// FIXED order -- four row classes (b mod 4), 32 rows per batch with all 32 loads in flight, then (s0 + s1) + (s2 + s3) -- shared by
// k_gn_solve, k_track_gn_fused and (re-stated on LDS rows) k_track_level, so every schedule gives the same bits.
// Rows outside [blk_first, blk_first + blk_count) were not written (crop window): they count as exact zeros in the same slots.
// (STRIDE: floats per partial row -- 32 for the 29 sums, 8 for the brightness moments of k_track_gn_ab)
template <int STRIDE = 32>
__device__ __forceinline__ double sum_partial_rows(const float* p, const int nblk, const int blk_first, const int blk_count)
{
    const int live0 = blk_count < 0 ? 0 : blk_first, live1 = blk_count < 0 ? nblk : blk_first + blk_count;
    double sg[DVO_SOLVE_GROUPS] = {0.0, 0.0, 0.0, 0.0};
    for (int b0 = 0; b0 < nblk; b0 += 8 * DVO_SOLVE_GROUPS) {  // 32 loads in flight per lane
        float v[DVO_SOLVE_GROUPS][8];
#pragma unroll
        for (int g = 0; g < DVO_SOLVE_GROUPS; g++)
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const int b = b0 + g + DVO_SOLVE_GROUPS * j;
                const bool live = (b >= live0) & (b < live1);
                const float x = p[(size_t)(live ? b : 0) * STRIDE];  // (always a valid address: no branch around the load)
                v[g][j] = live ? x : 0.0f;
            }
#pragma unroll
        for (int g = 0; g < DVO_SOLVE_GROUPS; g++)
#pragma unroll
            for (int j = 0; j < 8; j++)
                if (b0 + g < nblk) sg[g] += (double)v[g][j];  // (a class with no row left adds nothing, as before)
    }
    return (sg[0] + sg[1]) + (sg[2] + sg[3]);
}

// One row class g of sum_partial_rows() -- the rows b = g (mod 4) in increasing b, i.e. exactly the additions that function performs
// for sg[g], in its order -- with EVERY load of the class issued before the first addition (up to DVO_WIDE_BATCHES x 8 rows per lane:
// nblk <= 32 * DVO_WIDE_BATCHES).  One sequence gives a 32-lane team per class instead of one team for all four: a dvo_vo handle's
// finest level (300 partial rows) took ten dependent memory round trips here, ~15 us of its 20 us solve kernel; now one.
// (s0 + s1) + (s2 + s3) of the four results are the bits sum_partial_rows() returns.
#define DVO_WIDE_BATCHES 10
__device__ __forceinline__ double sum_partial_class(const float* p, const int nblk, const int blk_first, const int blk_count, const int g)
{
    const int live0 = blk_count < 0 ? 0 : blk_first, live1 = blk_count < 0 ? nblk : blk_first + blk_count;
    float v[DVO_WIDE_BATCHES][8];
#pragma unroll
    for (int bi = 0; bi < DVO_WIDE_BATCHES; bi++) {
        // (wave-uniform: batches past the last row issue no loads -- a wave holds at most 63 loads in flight, so the 80 of a full
        //  table are two memory round trips and the 24 of a 75-row level one: 4.0 -> 2 us of every single-stream iteration)
        if (32 * bi < nblk) {
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const int b = 32 * bi + g + DVO_SOLVE_GROUPS * j;
                const bool live = (b >= live0) & (b < live1);
                const float x = p[(size_t)(live ? b : 0) * 32];
                v[bi][j] = live ? x : 0.0f;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; j++) v[bi][j] = 0.0f;
        }
    }
    double sg = 0.0;
#pragma unroll
    for (int bi = 0; bi < DVO_WIDE_BATCHES; bi++)
#pragma unroll
        for (int j = 0; j < 8; j++)
            if (32 * bi < nblk && 32 * bi + g < nblk) sg += (double)v[bi][j];   // (the same zeros in the same slots as sum_partial_rows)
    return sg;
}

__global__ void __launch_bounds__(32 * DVO_SOLVE_SEQ) k_gn_solve(SolveArgs a)
{
    __shared__ double tot[DVO_SOLVE_SEQ][32];
    __shared__ double part[2][DVO_SOLVE_GROUPS][32];
    const int n_in = a.list_in ? a.list_in[0] : a.n_seq;  // sequences this launch handles
    // progress word in mapped host memory (adaptive schedule, Tracker::track): "iteration reached, n sequences were active".
    // Kept out of k_track_gn on purpose: that kernel sits exactly at its 72-VGPR budget and one more live value makes it spill.
    // Fine-grained host memory + a system-scope atomic store (sc0 sc1: written through, never parked in L2).  Relaxed on purpose:
    // the word is a hint for the host's launch schedule, no data is read on its strength, and a system-scope RELEASE here would
    // write back every dirty L2 line (the partial rows k_track_gn has just produced) once per launch.
    if (a.progress && blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_store(a.progress, n_in + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if ((int)blockIdx.x * DVO_SOLVE_SEQ >= n_in) return;
    // Everything this kernel needs from memory is requested up front (a fresh kernel starts with cold caches: each
    // dependent round trip costs ~2 us): lanes 0..7 the state of their sequence, every team its partial rows.
    const int my_slot = (int)blockIdx.x * DVO_SOLVE_SEQ + (int)threadIdx.x;   // (serial stage: threads 0..7)
    const bool serial = threadIdx.x < DVO_SOLVE_SEQ && my_slot < n_in;
    int my_seq = 0;
    if (serial) my_seq = a.list_in ? a.list_in[4 + my_slot] : my_slot;
    SeqState& st = a.state[my_seq];
    int was_active = 0, it_prev = 0;
    float xi[6] = {0, 0, 0, 0, 0, 0};
    double Tc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (serial) {
        was_active = st.active; it_prev = st.iter;
#pragma unroll
        for (int i = 0; i < 6; i++) xi[i] = st.xi[i];
#pragma unroll
        for (int i = 0; i < 12; i++) Tc[i] = st.Tc[i];
    }
    // stage one: second reduction of the workgroup partials, fixed order (bit-reproducible; k_track_level mirrors it)
    const int c = threadIdx.x & 31, team = threadIdx.x >> 5;
    const int t_slot = (int)blockIdx.x * DVO_SOLVE_SEQ + team;
    if (n_in <= 2 && a.nblk <= 32 * DVO_WIDE_BATCHES) {   // (workgroup-uniform) one or two sequences: a team per row class, one round trip
        const int ws = team >> 2, wg = team & 3;
        if (ws < n_in && c < 29) {
            const int t_seq = a.list_in ? a.list_in[4 + ws] : ws;
            part[ws][wg][c] = sum_partial_class(a.partials + (size_t)t_seq * a.nblk * 32 + c, a.nblk, a.blk_first, a.blk_count, wg);
        }
        __syncthreads();
        if (threadIdx.x < 64) {
            const int ts = threadIdx.x >> 5;
            tot[ts][c] = (ts < n_in && c < 29) ? (part[ts][0][c] + part[ts][1][c]) + (part[ts][2][c] + part[ts][3][c]) : 0.0;
        }
    } else if (t_slot < n_in && c < 29) {
        const int t_seq = a.list_in ? a.list_in[4 + t_slot] : t_slot;
        tot[team][c] = sum_partial_rows(a.partials + (size_t)t_seq * a.nblk * 32 + c, a.nblk, a.blk_first, a.blk_count);
    } else if (c >= 29) {
        tot[team][c] = 0.0;
    }
    __syncthreads();
    if (!serial) return;
    if (!a.ignore_active && was_active == 0) return;  // converged sequence: nothing to do
    Pose np;
    (void)solve_finish(a, my_seq, st, tot[threadIdx.x], a.ignore_active, it_prev, xi, Tc, np);
}

// SolveLane: what the serial lane holds when solve_gather returns true -- its sequence and that sequence's iteration count, twist and
// exp(+xi) as the state held them before this solve.  (The __shared__ rows stay in the kernels: _md and the _ab kernels add their own.)
struct SolveLane {
    int seq = 0, it_prev = 0;
    float xi[6] = {0, 0, 0, 0, 0, 0};
    double Tc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
};
// The slot of the track log a solve writes, and with it the slot of every term's own log
__device__ __forceinline__ int term_log_slot(const SolveArgs& a, const SolveLane& ln) { return a.ignore_active ? 0 : ln.it_prev; }

// solve_gather: everything of a solve kernel up to its serial tail, shared by k_gn_solve_rw, _ab and _z: the progress
// word, the serial lanes' state loads, the second reduction stage of slots 0 .. NSUM-1 into tot (wide form for one or two sequences,
// one team per sequence otherwise; slots NSUM .. 31 are exact zeros) and the barrier.  True for a lane that goes on to solve_finish:
// lanes 0..7 of wave 0, one live sequence each; ln is that sequence's.  Every other lane is done.
//   pre(seq):               a term's own load beside the serial lane's state loads (all requests go out up front)
//   mid(t_slot, c, team):   a term's own sums ahead of the barrier
// k_gn_solve is this function written out with NSUM = 29 and no callbacks, on purpose: its serial chain is the latency of every
// iteration of the default path, and built from this helper its instruction stream is not the one that was measured (the early
// returns move).  A change to the summation order or to the state loads is made here AND there; tools/isa_compare.py shows whether
// k_gn_solve moved.
template <int NSUM, class Pre, class Mid>
__device__ __forceinline__ bool solve_gather(const SolveArgs& a, double (*tot)[32], double (*part)[DVO_SOLVE_GROUPS][32], SolveLane& ln,
                                             Pre&& pre, Mid&& mid)
{
    const int n_in = a.list_in ? a.list_in[0] : a.n_seq;
    if (a.progress && blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_store(a.progress, n_in + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if ((int)blockIdx.x * DVO_SOLVE_SEQ >= n_in) return false;
    const int my_slot = (int)blockIdx.x * DVO_SOLVE_SEQ + (int)threadIdx.x;
    const bool serial = threadIdx.x < DVO_SOLVE_SEQ && my_slot < n_in;
    if (serial) ln.seq = a.list_in ? a.list_in[4 + my_slot] : my_slot;
    const SeqState& st = a.state[ln.seq];
    int was_active = 0;
    if (serial) {
        was_active = st.active; ln.it_prev = st.iter;
#pragma unroll
        for (int i = 0; i < 6; i++) ln.xi[i] = st.xi[i];
#pragma unroll
        for (int i = 0; i < 12; i++) ln.Tc[i] = st.Tc[i];
        pre(ln.seq);
    }
    const int c = threadIdx.x & 31, team = threadIdx.x >> 5;
    const int t_slot = (int)blockIdx.x * DVO_SOLVE_SEQ + team;
    if (n_in <= 2 && a.nblk <= 32 * DVO_WIDE_BATCHES) {
        const int ws = team >> 2, wg = team & 3;
        if (ws < n_in && c < NSUM) {
            const int t_seq = a.list_in ? a.list_in[4 + ws] : ws;
            part[ws][wg][c] = sum_partial_class(a.partials + (size_t)t_seq * a.nblk * 32 + c, a.nblk, a.blk_first, a.blk_count, wg);
        }
        __syncthreads();
        if (threadIdx.x < 64) {
            const int ts = threadIdx.x >> 5;
            tot[ts][c] = (ts < n_in && c < NSUM) ? (part[ts][0][c] + part[ts][1][c]) + (part[ts][2][c] + part[ts][3][c]) : 0.0;
        }
    } else if (t_slot < n_in && c < NSUM) {
        const int t_seq = a.list_in ? a.list_in[4 + t_slot] : t_slot;
        tot[team][c] = sum_partial_rows(a.partials + (size_t)t_seq * a.nblk * 32 + c, a.nblk, a.blk_first, a.blk_count);
    } else if (c >= NSUM) {
        tot[team][c] = 0.0;
    }
    if (t_slot < n_in) mid(t_slot, c, team);
    __syncthreads();
    if (!serial) return false;
    return a.ignore_active || was_active != 0;   // (a converged sequence has nothing to do)
}

// The serial lane's upkeep of its sequence's RobustEntry after solve_finish (k_gn_solve_rw, and k_gn_solve_ab with robust weights on):
// it records the s2 this iteration's tile kernel used (last_s2) and, with the adaptive scale, writes the entry of the next launch from
// this iteration's residual -- one fixed-point step of the IRLS scale: s2 = max(residual, floor2), plain when the residual is not > 0
// (the -1 sentinel of an iteration without pixels).  t: the sequence's 29 sums.  (Only this lane ever writes the sequence's entry, and
// solve_finish does not know the table: a caller may read used_s2 before or after it.)
__device__ __forceinline__ void robust_solve_update(const RobustSolve& rs, const int seq, const float used_s2, const double* t)
{
    rs.last_s2[seq] = used_s2;
    if (rs.adaptive) {
        const int n_valid = (int)t[28];
        const float residual = n_valid > 0 ? (float)t[27] / (float)n_valid : -1.0f;   // solve_finish's own expression: the logged bits
        const float s2 = residual > rs.floor2 ? residual : rs.floor2;
        rs.table[seq] = robust_entry(residual > 0.0f ? rs.kind : DVO_ROBUST_NONE, rs.param, s2);
    }
}

// The serial lane's solve_finish on its own row of tot (every term's solve kernel)
__device__ __forceinline__ void lane_solve_finish(const SolveArgs& a, SolveLane& ln, const double* t)
{
    Pose np;
    (void)solve_finish(a, ln.seq, a.state[ln.seq], t, a.ignore_active, ln.it_prev, ln.xi, ln.Tc, np);
}

// k_gn_solve_rw: k_gn_solve for a batch with robust residual weights: solve_gather, solve_finish, and the sequence's RobustEntry
// (robust_solve_update) with the s2 that was read beside the state.
__global__ void __launch_bounds__(32 * DVO_SOLVE_SEQ) k_gn_solve_rw(SolveArgs a, RobustSolve rs)
{
    __shared__ double tot[DVO_SOLVE_SEQ][32];
    __shared__ double part[2][DVO_SOLVE_GROUPS][32];
    SolveLane ln;
    float used_s2 = 0.0f;
    if (!solve_gather<29>(a, tot, part, ln, [&](int seq) { used_s2 = rs.table[seq].s2; }, [](int, int, int) {})) return;
    const double* t = tot[threadIdx.x];
    lane_solve_finish(a, ln, t);
    robust_solve_update(rs, ln.seq, used_s2, t);
}

// k_robust_begin: the RobustEntry table at the start of a tracking call, one thread per sequence.  Adaptive scale: every sequence starts
// plain (the first iteration of the coarsest level).  Given scale: s2 = s * s of the sequence's row (plain unless s is finite and > 0),
// or s2_all for every sequence (dvo_op_gn_step_robust).  last_s2 = 0: "not tracked", until a solve says otherwise.
__global__ void __launch_bounds__(256) k_robust_begin(RobustBeginArgs a)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_seq) return;
    float s2 = 0.0f;
    if (a.given) {
        s2 = a.s2_all;
        if (a.scales) {
            const float s = a.scales[i];
            s2 = (s > 0.0f && s < __builtin_inff()) ? s * s : 0.0f;
        }
    }
    a.table[i] = robust_entry(a.kind, a.param, s2);
    a.last_s2[i] = 0.0f;
}

// k_gn_solve_md: k_gn_solve_rw for the median scale.  Ahead of solve_gather's barrier the 32 lanes that summed a
// sequence's partial rows also read its 256 counts (8 consecutive bins per lane), keep them in hist_last (not the priming pair), zero
// the row for the next tile launch (ordered behind this kernel on the stream), scan the counts and select the median bin: n = the
// total, m = the smallest bin with cum(m) >= (n + 1) / 2.  The serial lane then runs solve_finish, records the s2 this iteration used
// and writes the next entry from (m, n): robust_entry(kind, param, median_s2(m, floor2)), plain when n == 0.  ms.prime: the priming
// pair -- the entry and prime_mn only.
__global__ void __launch_bounds__(32 * DVO_SOLVE_SEQ) k_gn_solve_md(SolveArgs a, RobustSolve rs, MedianSolve ms)
{
    __shared__ double tot[DVO_SOLVE_SEQ][32];
    __shared__ double part[2][DVO_SOLVE_GROUPS][32];
    __shared__ int sel[DVO_SOLVE_SEQ][2];
    SolveLane ln;
    float used_s2 = 0.0f;
    const auto select = [&](int t_slot, int c, int team) {
        const int t_seq = a.list_in ? a.list_in[4 + t_slot] : t_slot;
        uint4* row = reinterpret_cast<uint4*>(ms.hist + (size_t)t_seq * DVO_MEDIAN_BINS) + 2 * c;
        const uint4 v0 = row[0], v1 = row[1];
        if (!ms.prime) {
            uint4* keep = reinterpret_cast<uint4*>(ms.hist_last + (size_t)t_seq * DVO_MEDIAN_BINS) + 2 * c;
            keep[0] = v0; keep[1] = v1;
        }
        row[0] = make_uint4(0u, 0u, 0u, 0u); row[1] = make_uint4(0u, 0u, 0u, 0u);
        const unsigned v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
        unsigned mine = 0u;
#pragma unroll
        for (int i = 0; i < 8; i++) mine += v[i];
        unsigned incl = mine;   // inclusive scan over the team's 32 lanes
#pragma unroll
        for (int d = 1; d < 32; d <<= 1) {
            const unsigned up = __shfl_up(incl, d, 32);
            if (c >= d) incl += up;
        }
        const unsigned n = __shfl(incl, 31, 32);
        const unsigned target = (n + 1u) >> 1;
        int m = DVO_MEDIAN_BINS;
        unsigned cum = incl - mine;
        if (n != 0u && cum < target && target <= incl) {
#pragma unroll
            for (int i = 0; i < 8; i++) {   // the smallest bin of this lane whose cumulative count reaches the target
                cum += v[i];
                if (m == DVO_MEDIAN_BINS && cum >= target) m = 8 * c + i;
            }
        }
#pragma unroll
        for (int d = 16; d >= 1; d >>= 1) {
            const int o = __shfl_xor(m, d, 32);
            m = o < m ? o : m;
        }
        if (c == 0) { sel[team][0] = n != 0u ? m : -1; sel[team][1] = (int)n; }
    };
    if (!solve_gather<29>(a, tot, part, ln, [&](int seq) { used_s2 = rs.table[seq].s2; }, select)) return;
    const int my_seq = ln.seq;
    const double* t = tot[threadIdx.x];
    if (!ms.prime) {
        lane_solve_finish(a, ln, t);
        robust_solve_update(rs, my_seq, used_s2, t);   // (rs.adaptive = 0: last_s2 only)
    }
    const int m = sel[threadIdx.x][0], n = sel[threadIdx.x][1];
    rs.table[my_seq] = n > 0 ? robust_entry(rs.kind, rs.param, median_s2(m, rs.floor2)) : robust_entry(DVO_ROBUST_NONE, rs.param, 0.0f);
    if (ms.step_mn) { ms.step_mn[2 * my_seq] = m; ms.step_mn[2 * my_seq + 1] = n; }
    if (ms.prime) {
        ms.prime_mn[2 * my_seq] = m; ms.prime_mn[2 * my_seq + 1] = n;
        return;
    }
    const int it = term_log_slot(a, ln);
    if (ms.log && it < ms.log_its) {
        int* lg = ms.log + (((size_t)my_seq * ms.levels + a.level) * ms.log_its + it) * 3;
        lg[0] = __float_as_int(used_s2); lg[1] = m; lg[2] = n;
    }
}

// k_median_begin: the median scale's rows at the start of a tracking call, one workgroup per sequence: no counts, no kept histogram,
// no priming record.  (Beside k_robust_begin, which stays as it is and starts every sequence plain.)
__global__ void __launch_bounds__(DVO_MEDIAN_BINS) k_median_begin(MedianBeginArgs a)
{
    const size_t i = (size_t)blockIdx.x * DVO_MEDIAN_BINS + threadIdx.x;
    a.hist[i] = 0u;
    a.hist_last[i] = 0u;
    if (threadIdx.x < 2) a.prime_mn[2 * (size_t)blockIdx.x + threadIdx.x] = 0;
}

// The closed-form least-squares (a, b) of one iteration's brightness moments, in double: `e` becomes the new entry
// when the guards hold and keeps its value otherwise.  N = M0 with robust weights, else n_valid.
__device__ __forceinline__ void affine_next_entry(const AffineSolve& f, const int n_valid, const double N, const double* m, AffineEntry& e)
{
    const double M1 = m[1], M2 = m[2], M11 = m[3], M12 = m[4];
    const double det = N * M11 - M1 * M1;
    const double an = (N * M12 - M1 * M2) / det;
    const double bn = (M2 - an * M1) / N;
    const double inf = __builtin_inf();
    const bool finite = (an > -inf) & (an < inf) & (bn > -inf) & (bn < inf);   // (false for NaN)
    if (n_valid >= f.min_pixels && det > (double)f.min_contrast * N * M11 && finite && an >= (double)f.gain_min && an <= (double)f.gain_max) {
        e.a = (float)an; e.b = (float)bn;
    }
}

// The brightness moments of team `team`'s sequence, ahead of solve_gather's barrier (its `mid`): lanes 0..7 of the team sum them in
// double in the order of the 29 sums (every schedule: the order of sum_partial_rows).
__device__ __forceinline__ void affine_sum_moments(const SolveArgs& a, const AffineSolve& f, double (*mtot)[8], const int t_slot, const int c,
                                                   const int team)
{
    if (c < 8) {
        const int t_seq = a.list_in ? a.list_in[4 + t_slot] : t_slot;
        mtot[team][c] = sum_partial_rows<8>(f.moments + (size_t)t_seq * a.nblk * 8 + c, a.nblk, a.blk_first, a.blk_count);
    }
}

// Affine upkeep of one sequence and iteration by its serial lane, after solve_finish: records the entry this iteration's tile kernel
// used (last, and the affine log at slot `it`) and, in ESTIMATE mode, writes the next launch's entry from this iteration's moments m.
// N: m[0] with robust weights, else n_valid.  True for the priming pair (f.prime): the entry and prime_ab only, and the caller is done.
__device__ __forceinline__ bool affine_solve_update(const AffineSolve& f, const SolveArgs& a, const int seq, const int it, const int n_valid,
                                                    const double N, const double* m)
{
    const AffineEntry used = f.table[seq];
    AffineEntry next = used;
    if (f.estimate) affine_next_entry(f, n_valid, N, m, next);
    if (f.moments_out) {
        double* mo = f.moments_out + (size_t)seq * DVO_AFFINE_MOMENTS;
        mo[0] = N;
        for (int i = 1; i < DVO_AFFINE_MOMENTS; i++) mo[i] = m[i];
    }
    if (f.estimate) f.table[seq] = next;
    if (f.prime) {
        f.prime_ab[2 * seq] = next.a; f.prime_ab[2 * seq + 1] = next.b;
        return true;
    }
    if (f.log && it < f.log_its) {
        float* lg = f.log + (((size_t)seq * f.levels + a.level) * f.log_its + it) * 2;
        lg[0] = used.a; lg[1] = used.b;
    }
    f.last[2 * seq] = used.a; f.last[2 * seq + 1] = used.b;
    return false;
}

// Geometric record of one sequence and iteration by its serial lane, after solve_finish: slots 29 (sum rg^2) and 30 (n_geo) of its sums
// t go to sums_out, to the geometric log at slot `it` and to last.
__device__ __forceinline__ void geo_solve_record(const GeoSolve& z, const SolveArgs& a, const int seq, const int it, const double* t)
{
    const double S29 = t[29], n_geo = t[30];
    if (z.sums_out) { z.sums_out[2 * (size_t)seq] = n_geo; z.sums_out[2 * (size_t)seq + 1] = S29; }
    if (z.log && it < z.log_its) {
        float* lg = z.log + (((size_t)seq * z.levels + a.level) * z.log_its + it) * 2;
        lg[0] = (float)n_geo; lg[1] = (float)S29;
    }
    float* last = z.last + 4 * (size_t)seq;   // (n_geo, mean_sq, 1 = tracked, 0)
    last[0] = (float)n_geo; last[1] = n_geo > 0.0 ? (float)(S29 / n_geo) : 0.0f; last[2] = 1.0f;
}

// k_gn_solve_ab: k_gn_solve_rw for a batch with affine brightness compensation: solve_gather with the moments in mid, solve_finish,
// then the sequence's AffineEntry (affine_solve_update).  The pose first, the brightness entry after it: nothing of the closed form is
// live across the serial chain of solve_finish.  f.prime: the priming pair -- the entry and prime_ab only.  The RobustEntry is kept
// exactly as k_gn_solve_rw keeps it when robust weights are on too (f.robust).
__global__ void __launch_bounds__(32 * DVO_SOLVE_SEQ) k_gn_solve_ab(SolveArgs a, RobustSolve rs, AffineSolve f)
{
    __shared__ double tot[DVO_SOLVE_SEQ][32];
    __shared__ double part[2][DVO_SOLVE_GROUPS][32];
    __shared__ double mtot[DVO_SOLVE_SEQ][8];
    SolveLane ln;
    if (!solve_gather<29>(a, tot, part, ln, [](int) {}, [&](int t_slot, int c, int team) { affine_sum_moments(a, f, mtot, t_slot, c, team); })) return;
    const double* t = tot[threadIdx.x];
    if (!f.prime) lane_solve_finish(a, ln, t);
    const double* m = mtot[threadIdx.x];
    const int n_valid = (int)t[28];
    if (affine_solve_update(f, a, ln.seq, term_log_slot(a, ln), n_valid, f.robust ? m[0] : (double)n_valid, m)) return;
    if (f.robust) robust_solve_update(rs, ln.seq, rs.table[ln.seq].s2, t);
}

// k_gn_solve_z: k_gn_solve for a sensor-depth batch with the geometric term: solve_gather sums slots 29 (sum rg^2) and 30 (n_geo) of
// the partial rows beside the 29 in the same fixed order; the serial thread records them (geo_solve_record).  solve_finish reads slots
// 0..28 only: it solves the combined H and g, and n_valid, the residual and the stop tests stay photometric.
__global__ void __launch_bounds__(32 * DVO_SOLVE_SEQ) k_gn_solve_z(SolveArgs a, GeoSolve z)
{
    __shared__ double tot[DVO_SOLVE_SEQ][32];
    __shared__ double part[2][DVO_SOLVE_GROUPS][32];
    SolveLane ln;
    if (!solve_gather<31>(a, tot, part, ln, [](int) {}, [](int, int, int) {})) return;
    const double* t = tot[threadIdx.x];
    lane_solve_finish(a, ln, t);
    geo_solve_record(z, a, ln.seq, term_log_slot(a, ln), t);
}

// k_gn_solve_zab: k_gn_solve_z for a batch that also compensates brightness (k_track_gn_zab's partner): solve_gather sums the 31 slots
// and, in mid, the brightness moments; the serial lane runs solve_finish, records the geometric sums as k_gn_solve_z does and then keeps
// the AffineEntry as k_gn_solve_ab does without robust weights (N = n_valid).  The pose and the geometric record first, the closed form
// last: nothing of it is live across the serial chain of solve_finish.  f.prime: the priming pair -- the entry and prime_ab only.
__global__ void __launch_bounds__(32 * DVO_SOLVE_SEQ) k_gn_solve_zab(SolveArgs a, AffineSolve f, GeoSolve z)
{
    __shared__ double tot[DVO_SOLVE_SEQ][32];
    __shared__ double part[2][DVO_SOLVE_GROUPS][32];
    __shared__ double mtot[DVO_SOLVE_SEQ][8];
    SolveLane ln;
    if (!solve_gather<31>(a, tot, part, ln, [](int) {}, [&](int t_slot, int c, int team) { affine_sum_moments(a, f, mtot, t_slot, c, team); })) return;
    const double* t = tot[threadIdx.x];
    const int it = term_log_slot(a, ln);
    if (!f.prime) {
        lane_solve_finish(a, ln, t);
        geo_solve_record(z, a, ln.seq, it, t);
    }
    const int n_valid = (int)t[28];
    (void)affine_solve_update(f, a, ln.seq, it, n_valid, (double)n_valid, mtot[threadIdx.x]);
}

// k_affine_begin: the AffineEntry table at the start of a tracking call, one thread per sequence.  ESTIMATE: every sequence starts at
// (1, 0).  GIVEN: the sequence's row ((1, 0) unless finite with a > 0), or (a_all, b_all) for every sequence (dvo_op_gn_step_affine).
// last = (0, 0): "not tracked", until a solve says otherwise.
__global__ void __launch_bounds__(256) k_affine_begin(AffineBeginArgs a)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_seq) return;
    a.table[i] = a.rows ? affine_entry(a.rows[2 * i], a.rows[2 * i + 1]) : affine_entry(a.a_all, a.b_all);
    a.last[2 * i] = 0.0f; a.last[2 * i + 1] = 0.0f;
    a.prime_ab[2 * i] = 0.0f; a.prime_ab[2 * i + 1] = 0.0f;
}

// What solve_finish and lm_solve_finish share.  The iteration's row of the track log:
__device__ __forceinline__ void track_log_write(const SolveArgs& a, const int seq, const int it, const float residual, const double nrm,
                                                const int n_valid, const float* xi, const float* upd)
{
    if (a.log && it < DVO_MAX_ITERATIONS) {
        dvo_track_log& lg = a.log[seq];
        lg.n_iter[a.level] = it + 1;
        lg.residual[a.level][it] = residual;
        lg.update_norm[a.level][it] = (float)nrm;
        lg.n_valid[a.level][it] = n_valid;
#pragma unroll
        for (int i = 0; i < 6; i++) lg.xi_after[a.level][it][i] = xi[i];
#pragma unroll
        for (int i = 0; i < 6; i++) lg.xi_update[a.level][it][i] = upd[i];
    }
}
// The stop test of iteration `it`: the new active flag
__device__ __forceinline__ int solve_stays_active(const SolveArgs& a, const int it, const double nrm, const float residual)
{
    int active = 1;
    if (a.fixed_iterations > 0) {
        active = (it + 1 < a.fixed_iterations) ? 1 : 0;
    } else if (nrm < (double)a.min_update || residual < a.min_residual || it + 1 >= a.max_iterations) {
        active = 0;  // tracker.cpp:68-73 (the wall-clock term is disabled, D1)
    }
    return active;
}
// The end of a sequence's solve: its active flag, its slot on the next launch's list, the profile counters
__device__ __forceinline__ void solve_epilogue(const SolveArgs& a, const int seq, SeqState& st, const int active)
{
    st.active = active;
    if (active && a.list_out) a.list_out[4 + atomicAdd(&a.list_out[0], 1)] = seq;
    if (a.counters) {  // profile: evaluated pixels / sequence-iterations
        atomicAdd(&a.counters[0], (unsigned long long)a.level_pixels);
        atomicAdd(&a.counters[1], 1ull);
    }
}

// The serial part of one Tracker::track iteration (tracker.cpp:44-73) for one sequence, run by ONE thread: 6x6 solve,
// pose update, stop tests, log.  `tot` = the 29 sums in double; xi / Tc = the sequence's twist and exp(+xi) on entry,
// updated on return (and written to `st`); np = exp(-xi) after the update.  Returns the new active flag.
__device__ __forceinline__ int solve_finish(const SolveArgs& a, const int seq, SeqState& st, const double* tot, const int first,
                                            const int it_prev, float xi[6], double Tc[12], Pose& np)
{
    const int n_valid = (int)tot[28];
    const double sum_r2 = tot[27];
    float upd[6] = {0, 0, 0, 0, 0, 0};
    float residual = -1.0f;  // optimize.cpp:92-93
    if (n_valid > 0) {
        solve6(tot, tot + 21, upd);
        residual = (float)sum_r2 / (float)n_valid;  // optimize.cpp:98
    }
    if (a.dbg_stamp) a.dbg_stamp[0] = wall_clock64();
    // xi <- log(exp(xi) exp(upd)) unless NaN (tracker.cpp:46-51); pose <- exp(-xi) for Stuff::update (optimize.hpp:26-30)
    const bool updated = se3_update_pose(Tc, upd, xi, np);
    if (a.dbg_stamp) a.dbg_stamp[1] = wall_clock64();
    if (updated) {
#pragma unroll
        for (int i = 0; i < 6; i++) st.xi[i] = xi[i];
#pragma unroll
        for (int i = 0; i < 12; i++) st.Tc[i] = Tc[i];
        st.pose = np;
    }
    double nrm = 0.0;
#pragma unroll
    for (int i = 0; i < 6; i++) nrm += (double)upd[i] * (double)upd[i];
    nrm = sqrt(nrm);

    const int it = first ? 0 : it_prev;
    track_log_write(a, seq, it, residual, nrm, n_valid, xi, upd);
    if (a.result) {  // operator-level output (dvo_op_gn_step)
        dvo_gn_result& r = a.result[seq];
        for (int i = 0; i < 21; i++) r.H[i] = tot[i];
        for (int i = 0; i < 6; i++) { r.g[i] = tot[21 + i]; r.xi_update[i] = upd[i]; r.xi_next[i] = xi[i]; }
        r.sum_r2 = sum_r2;
        r.n_valid = n_valid;
        r.residual = residual;
    }
    st.iter = it + 1;
    const int active = solve_stays_active(a, it, nrm, residual);
    solve_epilogue(a, seq, st, active);
    return active | (updated ? 2 : 0);
}

// ------------------------------------------------------------------------------------------------
// k_track_gn_fused: one Tracker::track iteration in ONE launch, for a handful of sequences (a dvo_vo handle: one).  Every
// workgroup evaluates its tile exactly as k_track_gn does; the workgroup that finishes a sequence's LAST tile (an arrival ticket
// per sequence) then runs what k_gn_solve would: the second reduction stage in the same fixed order and solve_finish().  With one
// sequence the two-kernel form is nothing but latency -- two launches, two kernel boundaries and a cold-cache solve kernel per
// iteration; here it is one launch and the solve starts the moment the last partial row lands.  The price is the solve's register
// footprint (248 VGPRs, two waves per SIMD) for the whole kernel, which is irrelevant for the <= 1024 workgroups this path is used
// for and ruinous for a batch (measured in round 1): the host picks it per level (Tracker::track).
// Hand-off: partial rows are plain stores; each workgroup drains them (vmcnt(0)), barrier, lane 0 agent-scope release fence, then the
// ticket (agent-scope atomic add); the last arriver takes an agent-scope acquire fence (invalidates this CU's L1) before anyone
// in its workgroup loads the rows.  No workgroup ever waits for another one: nothing can hang.
// ------------------------------------------------------------------------------------------------
struct FusedArgs {
    int* ticket;        // [n_seq] arrival counters, zero between launches
    int* report;        // 2 ints of THIS (level, iteration): [0] sequences reported, [1] sequences still active afterwards
    int* progress;      // optional, fine-grained HOST memory: last reporter stores (active afterwards + 1)
    int n_seq;
};

template <int PPT, int G, bool T2D, bool PCAM>   // PCAM: per-sequence intrinsics (seq_intr)
__global__ void __launch_bounds__(256) k_track_gn_fused(GnArgs a, SolveArgs sa, FusedArgs f)
{
    __shared__ GnTileLds<PPT> lds;
    __shared__ double tot[32];
    __shared__ double part[DVO_SOLVE_GROUPS][32];
    __shared__ int last_s;
    const int tile_id = (int)blockIdx.x;                       // grid = n_seq * blk_count exactly
    const int seq = tile_id / a.blk_count, blk = a.blk_first + (tile_id - seq * a.blk_count);
    SeqState& st = sa.state[seq];
    auto report = [&](int active) {                              // one thread per sequence and launch
        if (active) __hip_atomic_fetch_add(&f.report[1], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int r = __hip_atomic_fetch_add(&f.report[0], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (r == f.n_seq - 1 && f.progress) {
            const int act = __hip_atomic_load(&f.report[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(f.progress, act + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    };
    const bool off = a.plan_action && a.plan_action[seq] != DVO_SEQ_TRACK;   // not tracked by this push (Batch plan)
    if (off || (!sa.ignore_active && st.active == 0)) {          // converged sequence: its first tile reports, nobody works
        if (blk == a.blk_first && threadIdx.x == 0) report(0);
        return;
    }
    const Pose pose = st.pose;                                   // wave-uniform -> scalar loads
    Intr cam;
    if constexpr (PCAM) cam = a.seq_k[seq];
    gn_tile<PPT, G, false, T2D, PCAM>(a, pose, seq, blk, lds, a.partials + ((size_t)seq * a.nblk + blk) * 32, cam);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // this wave's row stores have left
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int t = __hip_atomic_fetch_add(&f.ticket[seq], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = (t == a.blk_count - 1) ? 1 : 0;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(&f.ticket[seq], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
        }
        last_s = last;
    }
    __syncthreads();
    if (!last_s) return;
    if (a.nblk <= 32 * DVO_WIDE_BATCHES) {                        // a team per row class: every partial row requested at once
        const int c = threadIdx.x & 31, wg = (int)(threadIdx.x >> 5);
        if (wg < DVO_SOLVE_GROUPS && c < 29)
            part[wg][c] = sum_partial_class(a.partials + (size_t)seq * a.nblk * 32 + c, a.nblk, sa.blk_first, sa.blk_count, wg);
        __syncthreads();
        if (threadIdx.x < 32) tot[c] = c < 29 ? (part[0][c] + part[1][c]) + (part[2][c] + part[3][c]) : 0.0;
    } else if (threadIdx.x < 32) {
        const int c = threadIdx.x;
        tot[c] = c < 29 ? sum_partial_rows(a.partials + (size_t)seq * a.nblk * 32 + c, a.nblk, sa.blk_first, sa.blk_count) : 0.0;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    float xi[6];
    double Tc[12];
#pragma unroll
    for (int i = 0; i < 6; i++) xi[i] = st.xi[i];
#pragma unroll
    for (int i = 0; i < 12; i++) Tc[i] = st.Tc[i];
    Pose np;
    const int r = solve_finish(sa, seq, st, tot, sa.ignore_active, st.iter, xi, Tc, np);
    report(r & 1);
}

// ------------------------------------------------------------------------------------------------
// k_track_persist: ALL of Tracker::track (tracker.cpp:22-85: every level, every iteration) for ONE sequence in ONE launch -- what a
// dvo_vo handle runs per frame.  A fixed grid of co-resident workgroups strides over the tiles of the current level (gn_tile, the
// same code and tile size as k_track_gn: the same partial rows), every workgroup then takes an arrival ticket, and the LAST arriver
// does what k_gn_solve does (second reduction stage in the fixed order, solve_finish: 6x6 solve, pose composition, stop tests,
// log), decides what comes next (same level / next level / done) and publishes it with an epoch word; the other workgroups poll
// that word (s_sleep between polls) and go on.  Per iteration that replaces a kernel boundary (~4 us of launch floor + cold caches
// per launch, profiles/r03_single_*_trace.txt) by one ticket and one epoch hand-over.  Bit-identical to the launch-per-iteration
// schedules: same tiles, same summation order, same solve_finish().
// Safety: the grid is sized by the occupancy query (every workgroup resident), and EVERY wait is bounded -- a workgroup that polls
// `spin_limit` times without seeing its epoch marks the launch as given up and leaves; the others then run into the same limit.
// The host sees the mark instead of the result tag and re-runs the frame with the launch-per-iteration schedule.
// ------------------------------------------------------------------------------------------------
template <int PPT, int G, bool MONO>   // MONO: with the mono handle's keyframe decision as the tail (its own instance: the tail's two
__global__ void __launch_bounds__(256) k_track_persist(PersistArgs p)   // exponentials and logarithm otherwise weigh on the sensor-depth handle's solver)
{
    __shared__ GnTileLds<PPT> lds;
    __shared__ double tot[32];
    __shared__ double part[DVO_SOLVE_GROUPS][32];
    __shared__ int line_s[16];   // the control line as this workgroup last read / is about to write it
    __shared__ float mono_fx_s[6];   // (MONO) the frame's pose and keyframe flag, from the solver's thread to the age-table tail
    __shared__ int mono_need_s;
    __shared__ int gave_up_s;
    // Workgroup 0 only solves; workgroups 1 .. grid-1 evaluate tiles.  Nobody takes a contended atomic: a worker announces its tiles of
    // step s by storing (epoch0 + s + 1) into its OWN slot of `arrive`, the solver polls the slots (one lane each); the solver
    // publishes step s's outcome -- next level, status, and the new pose itself -- as ONE 64-byte line whose first word is
    // (epoch0 + s + 1), which the workers poll.  The sequence's serial state (xi, exp(xi), iteration count) never leaves the
    // solver's registers.
    int* const ctl = p.ctl;                 // [0] epoch, [1] next level, [2] status (0 go on, 1 done), [3..14] pose, [15] epoch again
    int* const arrive = p.ctl + 16;         // [grid]
    const int epoch0 = p.host_tag << 10;    // epoch numbers of this launch: never equal to a value an earlier launch left behind
    const int n_work = (int)gridDim.x - 1;
    int level = 0, step = 0;
    if (blockIdx.x != 0) {
        // ---------------------------------------------------------------------------------------------- tile workers
        const int me = (int)blockIdx.x - 1;
        for (;;) {
            if (threadIdx.x < 16) {   // the control line of this step (the first step is the identity pose on level 0: tracker.cpp:28)
                int v = 0;
                if (step == 0) {
                    v = (threadIdx.x == 3 || threadIdx.x == 7 || threadIdx.x == 11) ? __float_as_int(1.0f) : 0;   // (pose words 3..14: R row major, t)
                } else {
                    int polls = 0;
                    for (;;) {
                        v = __hip_atomic_load(&ctl[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        // The line is complete when its FIRST word (the epoch, stored last, after a release) and its LAST word (a copy
                        // of the epoch, stored with the payload) both carry this step's number: whatever order the 64 bytes were
                        // fetched in, a current first word means every store before the release had landed when it was read, and a
                        // current last word means the payload store itself had landed when the other end was read.
                        const int e0 = __builtin_amdgcn_readlane(v, 0), e15 = __builtin_amdgcn_readlane(v, 15);
                        if (e0 == epoch0 + step && e15 == epoch0 + step) break;
                        if (++polls > p.spin_limit) { v = (threadIdx.x == 2) ? 2 : v; break; }   // bounded: give up (status 2)
                    }
                }
                line_s[threadIdx.x] = v;
            }
            __syncthreads();
            const bool stamp = p.dbg && me == p.dbg_worker && threadIdx.x == 0 && step < 64;
            if (stamp) p.dbg[(64 + step) * 8 + 0] = wall_clock64();   // line seen
            const int status = line_s[2];
            if (status != 0) {
                if (status == 2 && threadIdx.x == 0 && p.host_result)
                    __hip_atomic_store(reinterpret_cast<int*>(p.host_result + 23), p.host_tag, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
                break;
            }
            level = line_s[1];
            Pose pose;
#pragma unroll
            for (int i = 0; i < 9; i++) pose.R[i] = __int_as_float(__builtin_amdgcn_readfirstlane(line_s[3 + i]));   // wave-uniform: SGPRs
#pragma unroll
            for (int i = 0; i < 3; i++) pose.t[i] = __int_as_float(__builtin_amdgcn_readfirstlane(line_s[12 + i]));
            const PersistLevel& L = p.lv[level];
            GnArgs a{};
            a.obj_gray = L.obj_gray; a.ref_gray = L.ref_gray; a.ref_depth = L.ref_depth; a.ref_wgt = L.ref_wgt; a.wgt_const = L.wgt_const;
            a.state = p.state; a.partials = p.partials; a.mask = nullptr;
            a.w = L.w; a.h = L.h; a.nblk = L.nblk; a.inv_w = L.inv_w; a.q256 = L.q256; a.r256 = L.r256; a.k = L.k; a.prm = L.prm;
            a.ignore_active = 1; a.list = nullptr; a.next_count = nullptr; a.n_seq = 1;
            a.blk_first = L.blk_first; a.blk_count = L.blk_count; a.t_shift = L.t_shift; a.x_org = L.x_org; a.y_org = L.y_org;
            a.tiles_x = L.tiles_x; a.tiles_y = 0; a.margin = 0;
            if (stamp) p.dbg[(64 + step) * 8 + 3] = wall_clock64();   // arguments and pose in registers
            for (int t = me; t < L.blk_count; t += n_work) {
                float* row = p.partials + (size_t)(L.blk_first + t) * 32;
                if constexpr (PPT == 4) {
                    if (L.t2d) gn_tile<PPT, G, false, true>(a, pose, 0, L.blk_first + t, lds, row, a.k);
                    else gn_tile<PPT, G, false, false>(a, pose, 0, L.blk_first + t, lds, row, a.k);
                } else {
                    gn_tile<PPT, G, false, false>(a, pose, 0, L.blk_first + t, lds, row, a.k);
                }
                __syncthreads();   // (the next tile reuses the LDS scratch)
            }
            if (stamp) p.dbg[(64 + step) * 8 + 4] = wall_clock64();   // gn_tile returned
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // this wave's row stores have left
            __syncthreads();
            if (stamp) p.dbg[(64 + step) * 8 + 1] = wall_clock64();   // tiles done
            if (threadIdx.x == 0) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");       // the rows, before the announcement
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __hip_atomic_store(&arrive[me], epoch0 + step + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (stamp) p.dbg[(64 + step) * 8 + 2] = wall_clock64();   // announced
            step++;
            __syncthreads();   // (line_s is rewritten in the next round)
        }
        return;
    }
    // -------------------------------------------------------------------------------------------------- the solver (workgroup 0)
    SeqState& st = p.state[0];
    float xi[6] = {0, 0, 0, 0, 0, 0};                       // thread 0's: the sequence's serial state (tracker.cpp:28: xi = 0)
    double Tc[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    int it_prev = 0, first = 1;
    if (threadIdx.x == 0 && p.log) {
        p.log[0].levels = p.levels;
        for (int l = 0; l < DVO_MAX_LEVELS; l++) p.log[0].n_iter[l] = 0;
    }
    for (;;) {
        const PersistLevel& L = p.lv[level];
        // every worker has announced step `step` (bounded polls: one lane per worker slot)
        if (threadIdx.x == 0) gave_up_s = 0;
        __syncthreads();
        const bool stamp = p.dbg && threadIdx.x == 0 && step < 64;
        if (stamp) p.dbg[step * 8 + 0] = wall_clock64();   // starts waiting
        for (int wk = (int)threadIdx.x; wk < n_work; wk += 256) {
            int polls = 0;
            while (__hip_atomic_load(&arrive[wk], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != epoch0 + step + 1) {
                if (++polls > p.spin_limit) { gave_up_s = 1; break; }
            }
        }
        if (stamp) p.dbg[step * 8 + 1] = wall_clock64();   // own slots seen
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // the workers' rows, after their announcements
        __syncthreads();
        if (stamp) p.dbg[step * 8 + 2] = wall_clock64();   // everybody arrived, fence done
        int status = 0, nl = level;
        if (gave_up_s) {
            status = 2;
        } else {
            const int c = threadIdx.x & 31, wg = (int)(threadIdx.x >> 5);
            if (wg < DVO_SOLVE_GROUPS && c < 29) part[wg][c] = sum_partial_class(p.partials + c, L.nblk, L.blk_first, L.blk_count, wg);
            __syncthreads();
            if (threadIdx.x < 32) tot[c] = c < 29 ? (part[0][c] + part[1][c]) + (part[2][c] + part[3][c]) : 0.0;
            __syncthreads();
        }
        if (stamp) p.dbg[step * 8 + 3] = wall_clock64();   // rows summed
        if (threadIdx.x == 0) {
            Pose np;
            if (status == 0) {
                SolveArgs sa{};
                sa.state = p.state; sa.partials = p.partials; sa.log = p.log; sa.result = nullptr; sa.counters = nullptr;
                sa.nblk = L.nblk; sa.level = level; sa.level_pixels = L.level_pixels;
                sa.max_iterations = p.max_iterations; sa.fixed_iterations = p.fixed_iterations;
                sa.min_update = p.min_update; sa.min_residual = p.min_residual;
                sa.ignore_active = first; sa.list_in = nullptr; sa.list_out = nullptr; sa.progress = nullptr; sa.n_seq = 1;
                sa.blk_first = L.blk_first; sa.blk_count = L.blk_count;
                if (stamp) sa.dbg_stamp = &p.dbg[(64 + step) * 8 + 5];   // (two free slots of worker 0's row)
                const int r = solve_finish(sa, 0, st, tot, first, it_prev, xi, Tc, np);
                it_prev = first ? 1 : it_prev + 1;       // (= st.iter)
                if (!(r & 2)) pose_from_xi(xi, -1.0f, np);   // update rejected (NaN, tracker.cpp:47-51): the pose stays exp(-xi) of the unchanged xi
                if (!(r & 1)) {            // the level stopped (tracker.cpp:68-73): next level, or done
                    nl = level + 1;
                    if (nl >= p.levels) {  // k_export_poses' work: twist + exp(xi) (system.hpp:92), also into the mapped host block
                        status = 1;
                        float T[16];
                        for (int i = 0; i < 6; i++) { st.xi[i] = xi[i]; p.xi_out[i] = xi[i]; }
                        se3_exp_f(xi, T);
                        for (int i = 0; i < 16; i++) p.T_out[i] = T[i];
                        float fxw[6], Tw[16];
                        int need = 0;
                        if (MONO && p.mono.enabled) {   // a mono handle: Frame::updateXi, needNewFrame and exp(xi) here, not in a launch of their own
                            MonoSeq& m = *p.mono.meta;
                            for (int i = 0; i < 6; i++) m.ref_xi[i] = p.mono.ref_xi[i];
                            m.ref_id = p.mono.ref_id; m.n_total = p.mono.n_total;
                            need = mono_decide_one(m, xi, p.mono.frame_id, p.mono.min_translation, p.mono.max_frames, fxw, Tw);
                            for (int i = 0; i < 6; i++) mono_fx_s[i] = fxw[i];
                            mono_need_s = need;
                        }
                        if (p.host_result) {
                            for (int i = 0; i < 6; i++) p.host_result[i] = xi[i];
                            for (int i = 0; i < 16; i++) p.host_result[6 + i] = T[i];
                            if (MONO && p.mono.enabled) {
                                for (int i = 0; i < 6; i++) p.host_result[24 + i] = fxw[i];
                                for (int i = 0; i < 16; i++) p.host_result[30 + i] = Tw[i];
                                reinterpret_cast<int*>(p.host_result)[46] = need;
                            }
                            __hip_atomic_store(reinterpret_cast<int*>(p.host_result + 22), p.host_tag, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
                        }
                    }
                }
            } else if (p.host_result) {
                __hip_atomic_store(reinterpret_cast<int*>(p.host_result + 23), p.host_tag, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
            if (stamp) { p.dbg[step * 8 + 4] = wall_clock64(); p.dbg[step * 8 + 6] = level; }   // solved
            line_s[0] = epoch0 + step + 1; line_s[1] = nl; line_s[2] = status; line_s[15] = epoch0 + step + 1;
            for (int i = 0; i < 9; i++) line_s[3 + i] = __float_as_int(np.R[i]);
            for (int i = 0; i < 3; i++) line_s[12 + i] = __float_as_int(np.t[i]);
        }
        __syncthreads();
        // publish: words 1..15 first, then (release) the epoch word the workers poll
        if (threadIdx.x >= 1 && threadIdx.x < 16) __hip_atomic_store(&ctl[threadIdx.x], line_s[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (threadIdx.x < 64) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (threadIdx.x == 0) __hip_atomic_store(&ctl[0], line_s[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (stamp) p.dbg[step * 8 + 5] = wall_clock64();   // published
        const int st_now = line_s[2], nl_now = line_s[1];
        __syncthreads();
        if (st_now != 0) {
            if constexpr (MONO) {
                // The frame is tracked and (thread 0, above) decided.  Not a keyframe: Mapper::update follows, and its per-keyframe
                // relative poses are this workgroup's last job -- one thread per keyframe of FrameHistory -- instead of a launch of their own.
                if (st_now == 1 && p.mono.enabled && p.mono.hist_xi && mono_need_s == 0) {
                    float fxi[6];
                    for (int k = 0; k < 6; k++) fxi[k] = mono_fx_s[k];   // (written by thread 0 before the barriers above)
                    for (int i = (int)threadIdx.x; i < p.mono.n_hist; i += 256) {
                        AgeEntry e;
                        age_entry_one(fxi, p.mono.hist_xi + (size_t)i * 6, i, e);
                        p.mono.ages[i] = e;
                    }
                    if (threadIdx.x == 0 && p.mono.zero_word) *p.mono.zero_word = 0;
                }
            }
            break;
        }
        first = (nl_now != level) ? 1 : 0;
        level = nl_now;
        step++;
    }
}

// ------------------------------------------------------------------------------------------------
// k_track_level: ALL iterations of one (coarse) pyramid level for one sequence in one launch -- the loop of
// tracker.cpp:42-74 on the device.  One workgroup per sequence: every iteration evaluates the level's live tiles with
// gn_tile() into LDS rows, sums them exactly as k_gn_solve does (same grouping, same order: bit-identical to the
// k_track_gn + k_gn_solve pair at the same PPT), and thread 0 runs solve_finish(); the workgroup leaves when its
// sequence stops.  A dependent kernel boundary costs ~8 us on this GPU, whatever the kernel does: for levels of a few
// tiles the 2 x max_iterations launches of the unfused schedule were all boundary; here there is one.
// ------------------------------------------------------------------------------------------------
template <int PPT, int G, bool PCAM>   // PCAM: per-sequence intrinsics (seq_intr)
__global__ void __launch_bounds__(256) k_track_level(GnArgs ga, SolveArgs sa)
{
    __shared__ GnTileLds<PPT> lds;
    __shared__ float rows[DVO_FUSED_MAX_TILES][32];
    __shared__ double part[8][32];
    __shared__ double tot[32];
    __shared__ float pose_s[12];
    __shared__ int flag_s;
    const int seq = blockIdx.x;
    if (ga.plan_action && ga.plan_action[seq] != DVO_SEQ_TRACK) return;   // not tracked by this push (Batch plan)
    Intr cam;
    if constexpr (PCAM) cam = ga.seq_k[seq];   // (ahead of every store and barrier: scalar loads)
    SeqState& st = sa.state[seq];
    // thread 0 owns the serial state of the sequence across iterations
    float xi[6];
    double Tc[12];
    int it_prev = 0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < 6; i++) xi[i] = st.xi[i];
#pragma unroll
        for (int i = 0; i < 12; i++) Tc[i] = st.Tc[i];
#pragma unroll
        for (int i = 0; i < 9; i++) pose_s[i] = st.pose.R[i];
#pragma unroll
        for (int i = 0; i < 3; i++) pose_s[9 + i] = st.pose.t[i];
    }
    __syncthreads();
    const int max_it = sa.fixed_iterations > 0 ? sa.fixed_iterations : sa.max_iterations;
    const int c = threadIdx.x & 31, grp = threadIdx.x >> 5;
    const int live0 = ga.blk_first, live1 = ga.blk_first + ga.blk_count;
    for (int it = 0; it < max_it; it++) {
        Pose pose;  // wave-uniform: broadcast from LDS into SGPRs
#pragma unroll
        for (int i = 0; i < 9; i++) pose.R[i] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, pose_s[i])));
#pragma unroll
        for (int i = 0; i < 3; i++) pose.t[i] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, pose_s[9 + i])));
        for (int blk = live0; blk < live1; blk++) gn_tile<PPT, G, false, false, PCAM>(ga, pose, seq, blk, lds, rows[blk], cam);
        __syncthreads();
        {  // second reduction stage, as in k_gn_solve (rows outside the live range are exact zeros)
            double s = 0.0;
            if (c < 29 && grp < DVO_SOLVE_GROUPS) {  // the grouping of k_gn_solve (its 128 threads)
                for (int b0 = grp; b0 < ga.nblk; b0 += 8 * DVO_SOLVE_GROUPS) {
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        const int b = b0 + DVO_SOLVE_GROUPS * j;
                        const bool live = (b >= live0) & (b < live1);
                        const float x = rows[live ? b : live0][c];  // (index always inside the array)
                        s += live ? (double)x : 0.0;
                    }
                }
            }
            part[grp][c] = s;
        }
        __syncthreads();
        if (threadIdx.x < 32)
            tot[c] = (part[0][c] + part[1][c]) + (part[2][c] + part[3][c]);
        __syncthreads();
        if (threadIdx.x == 0) {
            Pose np;
            const int r = solve_finish(sa, seq, st, tot, it == 0 ? 1 : 0, it_prev, xi, Tc, np);
            it_prev = it + 1;
            if (r & 2) {
#pragma unroll
                for (int i = 0; i < 9; i++) pose_s[i] = np.R[i];
#pragma unroll
                for (int i = 0; i < 3; i++) pose_s[9 + i] = np.t[i];
            }
            flag_s = r & 1;
        }
        __syncthreads();
        if (flag_s == 0) break;
    }
}

// k_track_begin: Tracker::track line 28 (xi = 0) for every sequence
__global__ void __launch_bounds__(256) k_track_begin(SeqState* state, dvo_track_log* log, int n_seq, int levels)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n_seq) return;
    SeqState& st = state[s];
    for (int i = 0; i < 6; i++) st.xi[i] = 0.0f;
    for (int i = 0; i < 9; i++) st.pose.R[i] = (i % 4 == 0) ? 1.0f : 0.0f;
    for (int i = 0; i < 3; i++) st.pose.t[i] = 0.0f;
    for (int i = 0; i < 12; i++) st.Tc[i] = (i < 9 && i % 4 == 0) ? 1.0 : 0.0;
    st.active = 1;
    st.iter = 0;
    if (log) {
        log[s].levels = levels;
        for (int l = 0; l < DVO_MAX_LEVELS; l++) log[s].n_iter[l] = 0;
    }
}

// k_plan: the actions of one Batch push (dvo_batch_set_actions), one thread per sequence.  Resolves the effective action and status,
// updates has_ref, resets every SeqState and log as k_track_begin does (active only for the sequences that track), and compacts
// the tracked sequences into one list per sub-batch (the Tracker::work_list format, local ids): workgroup-local slots from LDS
// counters, one global atomic per (workgroup, sub-batch).  List order is irrelevant to the results (as in k_gn_solve).
__global__ void __launch_bounds__(256) k_plan(PlanArgs a)
{
    __shared__ int cnt[8], base[8];
    const int s = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (threadIdx.x < 8) cnt[threadIdx.x] = 0;
    if (blockIdx.x == 0 && (int)threadIdx.x < a.n_sub) a.lists_clear[(size_t)threadIdx.x * a.list_stride] = 0;
    __syncthreads();
    int sub = 0, local = -1, pos = 0;
    if (s < a.n_seq) {
        const int req = a.actions ? (int)a.actions[s] : DVO_SEQ_TRACK;
        // a reference belongs to the camera it was taken with: a sequence whose intrinsics change at this push has none
        const int changed = a.cam_changed ? (int)a.cam_changed[s] : 0;
        const int had = a.has_ref[s] != 0 && !changed;
        int eff, status;
        if (req == DVO_SEQ_TRACK && had) { eff = DVO_SEQ_TRACK; status = DVO_SEQ_TRACKED; }
        else if (req == DVO_SEQ_TRACK || req == DVO_SEQ_RESTART) { eff = DVO_SEQ_RESTART; status = DVO_SEQ_STARTED; }
        else { eff = DVO_SEQ_SKIP; status = req == DVO_SEQ_SKIP ? DVO_SEQ_SKIPPED : DVO_SEQ_BAD_ACTION; }
        a.eff[s] = (uint8_t)eff;
        a.status[s] = status;
        if (eff != DVO_SEQ_SKIP) a.has_ref[s] = 1;
        else if (changed) a.has_ref[s] = 0;
        SeqState& st = a.state[s];
        for (int i = 0; i < 6; i++) st.xi[i] = 0.0f;
        for (int i = 0; i < 9; i++) st.pose.R[i] = (i % 4 == 0) ? 1.0f : 0.0f;
        for (int i = 0; i < 3; i++) st.pose.t[i] = 0.0f;
        for (int i = 0; i < 12; i++) st.Tc[i] = (i < 9 && i % 4 == 0) ? 1.0 : 0.0;
        st.active = eff == DVO_SEQ_TRACK ? 1 : 0;
        st.iter = 0;
        a.log[s].levels = a.levels;
        for (int l = 0; l < DVO_MAX_LEVELS; l++) a.log[s].n_iter[l] = 0;
        if (eff == DVO_SEQ_TRACK) {   // sub-batch k holds [n_seq * k / n_sub, n_seq * (k + 1) / n_sub) (Tracker::sub_first)
            int q0 = 0;
            for (int k = 1; k < a.n_sub; k++) {
                const int f = (int)(((long long)a.n_seq * k) / a.n_sub);
                if (s >= f) { sub = k; q0 = f; }
            }
            local = s - q0;
            pos = atomicAdd(&cnt[sub], 1);
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < a.n_sub && cnt[threadIdx.x] > 0)
        base[threadIdx.x] = atomicAdd(&a.lists[(size_t)threadIdx.x * a.list_stride], cnt[threadIdx.x]);
    if (a.ready && threadIdx.x == 0) {   // the adaptive schedule's word: the last workgroup to finish publishes the tracked count
        int n = 0;
        for (int k = 0; k < a.n_sub && k < 8; k++) n += cnt[k];
        __hip_atomic_fetch_add(&a.tally[0], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int t = __hip_atomic_fetch_add(&a.tally[1], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (t == (int)gridDim.x - 1) {
            const int total = __hip_atomic_load(&a.tally[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            a.tally[0] = 0; a.tally[1] = 0;   // (zero for the next launch: kernel boundary)
            __hip_atomic_store(a.ready, total + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    __syncthreads();
    if (local >= 0) a.lists[(size_t)sub * a.list_stride + 4 + base[sub] + pos] = local;
}

// k_set_pose: load a caller-supplied twist (operator-level gn_step / probes)
__global__ void k_set_pose(SeqState* state, const float* xi, int n_seq)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_seq) return;
    float x[6];
    double xd[6], R[9], t[3];
    for (int i = 0; i < 6; i++) { x[i] = xi[s * 6 + i]; state[s].xi[i] = x[i]; xd[i] = x[i]; }
    pose_from_xi(x, -1.0f, state[s].pose);
    se3_exp_d(xd, R, t);
    for (int i = 0; i < 9; i++) state[s].Tc[i] = R[i];
    for (int i = 0; i < 3; i++) state[s].Tc[9 + i] = t[i];
    state[s].active = 1;
    state[s].iter = 0;
}

// k_seed_pose: the start pose of a sensor-depth push (dvo_batch_set_pose_guess_mode), after k_track_begin / k_plan.  History: the
// relative twist of the sequence's last TRACKED push since its last start (a RESTART zeroes it, a SKIP keeps it).
__global__ void __launch_bounds__(256) k_seed_pose(PoseSeedArgs a)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= a.n_seq) return;
    float* vel = a.hist + (size_t)s * 12;
    const int pe = a.prev_eff[s];
    if (pe == DVO_SEQ_TRACK) for (int i = 0; i < 6; i++) vel[i] = a.last_xi[(size_t)s * 6 + i];
    else if (pe == DVO_SEQ_RESTART) for (int i = 0; i < 6; i++) vel[i] = 0.0f;
    const int eff = a.eff ? (int)a.eff[s] : a.all_eff;
    a.prev_eff[s] = (uint8_t)eff;
    float x[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (eff == DVO_SEQ_TRACK) {
        if (a.mode == DVO_GUESS_GIVEN && a.rows) for (int i = 0; i < 6; i++) x[i] = a.rows[(size_t)s * 6 + i];
        else if (a.mode == DVO_GUESS_CONSTANT_VELOCITY) for (int i = 0; i < 6; i++) x[i] = vel[i];
    }
    seed_state(a.state[s], x, a.start + (size_t)s * 6);
}

// solve6's choice of solve6_pinv (dvo_math.h), restated operation for operation (the build does not contract, so the same
// expressions give the same bits): the largest diagonal entry (NaN entries skipped) is > 0 and an LDL^T pivot is <= 1e-12 times it.
// (Factoring this out of solve6 changed the instruction streams of the solve kernels, so it is kept apart.)
__device__ __forceinline__ bool solve6_takes_pinv(const double H[21])
{
    double maxd = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) maxd = H[tri(i, i)] > maxd ? H[tri(i, i)] : maxd;
    if (!(maxd > 0.0)) return false;
    double L[6][6], d[6];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double dj = H[tri(j, j)];
#pragma unroll
        for (int k = 0; k < j; k++) dj -= L[j][k] * L[j][k] * d[k];
        ok = ok && (dj > 1e-12 * maxd);
        d[j] = dj;
        const double inv = 1.0 / dj;
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            double v = H[tri(j, i)];
#pragma unroll
            for (int k = 0; k < j; k++) v -= L[i][k] * L[j][k] * d[k];
            L[i][j] = v * inv;
        }
    }
    return !ok;
}

// k_track_quality: one dvo_track_quality per sequence from the finest level's last solve (include/dvo.h).  Runs once per
// read, not per push.  jacobi_eig6 is used as it is: inlined here, its loops unroll and A, V stay in registers (170 VGPRs, no
// scratch: two waves per SIMD, plenty for n_seq threads).
__global__ void __launch_bounds__(64) k_track_quality(QualityArgs a)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= a.n_seq) return;
    dvo_track_quality& q = a.out[s];
    const int status = a.status ? a.status[s] : a.all_status;
    const int L = a.levels - 1;
    const double nan = __builtin_nan("");
    q.struct_size = (int)sizeof(dvo_track_quality);
    q.status = status;
    if (status != DVO_SEQ_TRACKED) {   // no solve of this push: the empty record
        q.flags = 0; q.n_valid = 0;
        for (int l = 0; l < DVO_MAX_LEVELS; l++) q.n_iter[l] = 0;
        q.residual = -1.0f; q.update_norm = 0.0f; q.sum_r2 = 0.0;
        for (int i = 0; i < 21; i++) { q.H[i] = 0.0; q.covariance[i] = nan; }
        for (int i = 0; i < 6; i++) { q.g[i] = 0.0; q.eigenvalues[i] = nan; }
        return;
    }
    const dvo_track_log& lg = a.log[s];
    const dvo_gn_result& r = a.rec[s];
    for (int l = 0; l < DVO_MAX_LEVELS; l++) q.n_iter[l] = l <= L ? lg.n_iter[l] : 0;
    int it = lg.n_iter[L] - 1;   // the finest level's last iteration (every TRACKED sequence solves it at least once)
    it = it < 0 ? 0 : (it < DVO_MAX_ITERATIONS ? it : DVO_MAX_ITERATIONS - 1);
    const int n_valid = r.n_valid;
    q.n_valid = n_valid;
    q.residual = r.residual;
    q.update_norm = lg.update_norm[L][it];
    q.sum_r2 = r.sum_r2;
    double H[21], A[36], V[36];
    bool finite = isfinite(r.sum_r2);
    for (int i = 0; i < 21; i++) { H[i] = r.H[i]; q.H[i] = H[i]; finite = finite && isfinite(H[i]); }
    for (int i = 0; i < 6; i++) { q.g[i] = r.g[i]; finite = finite && isfinite(r.g[i]); }
    // flags: solve_finish's stop tests on the same values (|upd| in double, as there)
    int flags = n_valid == 0 ? DVO_QUALITY_NO_VALID : 0;
    double nrm = 0.0;
    bool upd_finite = true;
    for (int i = 0; i < 6; i++) {
        const float u = lg.xi_update[L][it][i];
        nrm += (double)u * (double)u;
        upd_finite = upd_finite && isfinite(u);
    }
    nrm = sqrt(nrm);
    if (!upd_finite) flags |= DVO_QUALITY_NOT_FINITE;
    if (a.fixed_iterations <= 0) {
        if (nrm < (double)a.min_update || r.residual < a.min_residual) flags |= DVO_QUALITY_CONVERGED;
        else if (it + 1 >= a.max_iterations) flags |= DVO_QUALITY_CAPPED;
    }
    const bool rank_def = n_valid > 0 && solve6_takes_pinv(H);   // (solve_finish calls solve6 only when n_valid > 0)
    if (rank_def) flags |= DVO_QUALITY_RANK_DEFICIENT;
    q.flags = flags;
    // eigen-decomposition H = V diag(lambda) V^T (Jacobi, double) and covariance s2 V diag(1 / lambda) V^T
    for (int i = 0, k = 0; i < 6; i++)
        for (int j = i; j < 6; j++, k++) { A[6 * i + j] = H[k]; A[6 * j + i] = H[k]; }
    jacobi_eig6(A, V);
    double lam[6];
    for (int i = 0; i < 6; i++) lam[i] = finite ? A[7 * i] : nan;
    bool cov_ok = finite && n_valid > 6 && !rank_def;
    for (int i = 0; i < 6; i++) cov_ok = cov_ok && lam[i] > 0.0;
    const double s2 = cov_ok ? r.sum_r2 / (double)(n_valid - 6) : nan;
    for (int i = 0, k = 0; i < 6; i++)
        for (int j = i; j < 6; j++, k++) {
            double c = 0.0;
            for (int e = 0; e < 6; e++) c += V[6 * i + e] * V[6 * j + e] / lam[e];
            q.covariance[k] = cov_ok ? s2 * c : nan;
        }
    for (int i = 1; i < 6; i++)   // ascending
        for (int j = i; j > 0 && lam[j] < lam[j - 1]; j--) { const double t = lam[j]; lam[j] = lam[j - 1]; lam[j - 1] = t; }
    for (int i = 0; i < 6; i++) q.eigenvalues[i] = lam[i];
}

// k_export_poses: relative twist + exp(xi) 4x4 (system.hpp:92) per sequence
// host_result (optional, fine-grained mapped HOST memory, one sequence): the same 22 floats, then a sequence word written with a
// system-scope release store -- the caller's thread polls it instead of queueing a device-to-host copy and waiting for the stream
// (a dvo_vo handle returns one pose per call: three small copies + a stream synchronisation were ~55 us of every frame).
__global__ void k_export_poses(const SeqState* state, float* xi_out, float* T_out, int n_seq, float* host_result, int host_tag)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_seq) return;
    float x[6], T[16];
    for (int i = 0; i < 6; i++) { x[i] = state[s].xi[i]; xi_out[s * 6 + i] = x[i]; }
    se3_exp_f(x, T);
    for (int i = 0; i < 16; i++) T_out[s * 16 + i] = T[i];
    if (host_result && s == 0) {
        for (int i = 0; i < 6; i++) host_result[i] = x[i];
        for (int i = 0; i < 16; i++) host_result[6 + i] = T[i];
        __hip_atomic_store(reinterpret_cast<int*>(host_result + 22), host_tag, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// k_se3: device evaluation of the double-precision pose algebra (parity op): op 0 exp, 1 log, 2 concatenate
__global__ void k_se3(int op, const float* in_a, const float* in_b, float* out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (op == 0) {
        float xi[6], T[16];
        for (int i = 0; i < 6; i++) xi[i] = in_a[i];
        se3_exp_f(xi, T);
        for (int i = 0; i < 16; i++) out[i] = T[i];
    } else if (op == 1) {
        float T[16], xi[6];
        for (int i = 0; i < 16; i++) T[i] = in_a[i];
        se3_log_f(T, xi);
        for (int i = 0; i < 6; i++) out[i] = xi[i];
    } else {
        float x[6], y[6], o[6];
        for (int i = 0; i < 6; i++) { x[i] = in_a[i]; y[i] = in_b[i]; }
        se3_concatenate_f(x, y, o);
        for (int i = 0; i < 6; i++) out[i] = o[i];
    }
}

// k_pose_algebra: the pieces of the serial double chain that ends every Gauss-Newton iteration (solve6, se3_update_pose) and of the
// mapping side's pose bookkeeping (se3_concatenate_f, pose_from_xi), one case per thread, doubles in and out so that nothing is
// rounded on the way (parity op, like k_se3: tests/test_gpu_pose_algebra.py holds it to a multi-precision reference).  Rows per case
// (pose_algebra_row): op 0 se3_exp_d  xi[6] -> R[9] t[3];  1 se3_log_d  R[9] t[3] -> xi[6];  2 se3_concatenate_f  a[6] b[6] -> out[6];
// 3 se3_update_pose on the state seed_state sets up for xi  xi[6] upd[6] -> ok, xi'[6], Tc'[12], pose R[9] t[3];
// 4 solve6  H[21] g[6] -> x[6], solve6_takes_pinv;  5 jacobi_eig6  H[21] -> diag[6], V[36].
__global__ void __launch_bounds__(64) k_pose_algebra(int op, int n, const double* __restrict__ in, double* __restrict__ out)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    int ni, no;
    pose_algebra_row(op, ni, no);
    const double* p = in + (size_t)i * ni;
    double* o = out + (size_t)i * no;
    if (op == 0) {
        double xi[6], R[9], t[3];
        for (int k = 0; k < 6; k++) xi[k] = p[k];
        se3_exp_d(xi, R, t);
        for (int k = 0; k < 9; k++) o[k] = R[k];
        for (int k = 0; k < 3; k++) o[9 + k] = t[k];
    } else if (op == 1) {
        double R[9], t[3], xi[6];
        for (int k = 0; k < 9; k++) R[k] = p[k];
        for (int k = 0; k < 3; k++) t[k] = p[9 + k];
        se3_log_d(R, t, xi);
        for (int k = 0; k < 6; k++) o[k] = xi[k];
    } else if (op == 2) {
        float a[6], b[6], c[6];
        for (int k = 0; k < 6; k++) { a[k] = (float)p[k]; b[k] = (float)p[6 + k]; }
        se3_concatenate_f(a, b, c);
        for (int k = 0; k < 6; k++) o[k] = c[k];
    } else if (op == 3) {
        float xi[6], upd[6];
        double xd[6], Tc[12];
        Pose pose;
        for (int k = 0; k < 6; k++) { xi[k] = (float)p[k]; upd[k] = (float)p[6 + k]; xd[k] = xi[k]; }
        pose_from_xi(xi, -1.0f, pose);   // (seed_state, dvo_kernels.h)
        se3_exp_d(xd, Tc, Tc + 9);
        o[0] = se3_update_pose(Tc, upd, xi, pose) ? 1.0 : 0.0;
        for (int k = 0; k < 6; k++) o[1 + k] = xi[k];
        for (int k = 0; k < 12; k++) o[7 + k] = Tc[k];
        for (int k = 0; k < 9; k++) o[19 + k] = pose.R[k];
        for (int k = 0; k < 3; k++) o[28 + k] = pose.t[k];
    } else if (op == 4) {
        double H[21], g[6];
        float x[6];
        for (int k = 0; k < 21; k++) H[k] = p[k];
        for (int k = 0; k < 6; k++) g[k] = p[21 + k];
        solve6(H, g, x);
        for (int k = 0; k < 6; k++) o[k] = x[k];
        o[6] = solve6_takes_pinv(H) ? 1.0 : 0.0;
    } else {
        double A[36], V[36];
        for (int r = 0, k = 0; r < 6; r++)
            for (int c = r; c < 6; c++, k++) { A[6 * r + c] = p[k]; A[6 * c + r] = p[k]; }
        jacobi_eig6(A, V);
        for (int k = 0; k < 6; k++) o[k] = A[7 * k];
        for (int k = 0; k < 36; k++) o[6 + k] = V[k];
    }
}

// ------------------------------------------------------------------------------------------------
// Step control (dvo_batch_set_step_control; the contract is in include/dvo.h): damped Gauss-Newton with step acceptance.
// (Kept behind every older kernel of this file on purpose: the device code of the kernels above is then laid out as it was.)
// lm_solve_finish: solve_finish for a batch with step control, by ONE thread per sequence.  `tot` = the 29 sums of the evaluation at the
// pose the state holds (xi / Tc on entry).  It decides (FIRST / ACCEPT / REJECT against the sequence's entry, float32 and integers),
// selects the 27 sums of whichever evaluation the entry now holds into ONE set, the lane's own row `tot` (overwritten) -- the entry is
// written before the serial chain, so no second system is live across solve6 and the SE(3) chain -- damps the diagonal, solves and
// composes the trial pose from the entry's Tc.  A sequence that stays active gets the trial pose, one that stops the accepted pose, read back from the entry.
// Shared by k_gn_solve_lm and k_lm_step (dvo_op_lm_step).
__device__ __forceinline__ void lm_solve_finish(const SolveArgs& a, const LmSolve& lm, const int seq, SeqState& st, double* tot,
                                                const int first, const int it_prev, float (&xi)[6], double (&Tc)[12])
{
    dvo_lm_entry& e = lm.table[seq];
    const int n_valid = (int)tot[28];
    const float residual = n_valid > 0 ? (float)tot[27] / (float)n_valid : -1.0f;   // solve_finish's own expression: the logged bits
    float lambda = e.lambda;
    int n_acc = e.n_valid;
    float res_acc = e.residual;
    int decision = DVO_LM_FIRST;
    if (!first) {
        const bool ok = n_valid > 0 && (float)n_valid >= lm.min_valid_fraction * (float)n_acc && residual <= res_acc;   // (false for NaN)
        decision = ok ? DVO_LM_ACCEPT : DVO_LM_REJECT;
        lambda = ok ? lambda * lm.lambda_down : fminf(fmaxf(lambda, lm.lambda_floor) * lm.lambda_up, lm.lambda_max);
    }
    double* S = tot;   // (the lane's own row: the system lives there, as in solve_finish, so solve6's out-of-line branch needs no copy)
    double sum_r2;
    if (decision != DVO_LM_REJECT) {   // this evaluation becomes the entry
#pragma unroll
        for (int i = 0; i < 21; i++) e.H[i] = S[i];
#pragma unroll
        for (int i = 0; i < 6; i++) { e.g[i] = S[21 + i]; e.xi[i] = xi[i]; }
#pragma unroll
        for (int i = 0; i < 12; i++) e.Tc[i] = Tc[i];
#pragma unroll
        for (int i = 0; i < 9; i++) e.pose[i] = st.pose.R[i];
#pragma unroll
        for (int i = 0; i < 3; i++) e.pose[9 + i] = st.pose.t[i];
        sum_r2 = tot[27]; n_acc = n_valid; res_acc = residual;
        e.sum_r2 = sum_r2; e.n_valid = n_acc; e.residual = res_acc;
    } else {                           // the entry stays: step from it again, with more damping
#pragma unroll
        for (int i = 0; i < 21; i++) S[i] = e.H[i];
#pragma unroll
        for (int i = 0; i < 6; i++) { S[21 + i] = e.g[i]; xi[i] = e.xi[i]; }
#pragma unroll
        for (int i = 0; i < 12; i++) Tc[i] = e.Tc[i];
        sum_r2 = e.sum_r2;
    }
    e.lambda = lambda;
    if (a.result) {  // the quality record: the accepted sums (the step and the pose follow below)
        dvo_gn_result& r = a.result[seq];
        for (int i = 0; i < 21; i++) r.H[i] = S[i];
        for (int i = 0; i < 6; i++) r.g[i] = S[21 + i];
        r.sum_r2 = sum_r2;
        r.n_valid = n_acc;
        r.residual = res_acc;
    }
    const double damp = 1.0 + (double)lambda;
    S[0] *= damp; S[6] *= damp; S[11] *= damp; S[15] *= damp; S[18] *= damp; S[20] *= damp;   // the diagonal of the upper triangle
    float upd[6] = {0, 0, 0, 0, 0, 0};
    if (n_acc > 0) solve6(S, S + 21, upd);
    Pose np;
    const bool updated = se3_update_pose(Tc, upd, xi, np);   // xi / Tc: the accepted pose on entry, the trial pose when it returns true
    double nrm = 0.0;
#pragma unroll
    for (int i = 0; i < 6; i++) nrm += (double)upd[i] * (double)upd[i];
    nrm = sqrt(nrm);
    const int it = first ? 0 : it_prev;
    int active = solve_stays_active(a, it, nrm, res_acc);
    if (!updated || !(nrm < __builtin_inf())) active = 0;   // a non-finite update ends the level
    if (active) {
#pragma unroll
        for (int i = 0; i < 6; i++) st.xi[i] = xi[i];
#pragma unroll
        for (int i = 0; i < 12; i++) st.Tc[i] = Tc[i];
        st.pose = np;
    } else {         // the level ends on the accepted pose
#pragma unroll
        for (int i = 0; i < 6; i++) { xi[i] = e.xi[i]; st.xi[i] = xi[i]; }
#pragma unroll
        for (int i = 0; i < 12; i++) st.Tc[i] = e.Tc[i];
#pragma unroll
        for (int i = 0; i < 9; i++) st.pose.R[i] = e.pose[i];
#pragma unroll
        for (int i = 0; i < 3; i++) st.pose.t[i] = e.pose[9 + i];
    }
    track_log_write(a, seq, it, residual, nrm, n_valid, xi, upd);
    if (a.result) {
        dvo_gn_result& r = a.result[seq];
        for (int i = 0; i < 6; i++) { r.xi_update[i] = upd[i]; r.xi_next[i] = xi[i]; }
    }
    if (lm.log && it < lm.log_its) {
        int* lg = lm.log + (((size_t)seq * lm.levels + a.level) * lm.log_its + it) * 2;
        lg[0] = __float_as_int(lambda); lg[1] = decision;
    }
    dvo_lm_record& rec = lm.last[seq];
    if (decision == DVO_LM_FIRST) rec.n_first += 1;
    else if (decision == DVO_LM_ACCEPT) rec.n_accepted += 1;
    else rec.n_rejected += 1;
    rec.lambda = lambda;
    if (a.level == lm.levels - 1) rec.residual = res_acc;
    if (lm.upd_out) {
#pragma unroll
        for (int i = 0; i < 6; i++) lm.upd_out[6 * (size_t)seq + i] = upd[i];
    }
    if (lm.decision_out) lm.decision_out[seq] = decision;
    st.iter = it + 1;
    solve_epilogue(a, seq, st, active);
}

// k_gn_solve_lm: k_gn_solve for a batch with step control: solve_gather, then lm_solve_finish.
__global__ void __launch_bounds__(32 * DVO_SOLVE_SEQ) k_gn_solve_lm(SolveArgs a, LmSolve lm)
{
    __shared__ double tot[DVO_SOLVE_SEQ][32];
    __shared__ double part[2][DVO_SOLVE_GROUPS][32];
    SolveLane ln;
    if (!solve_gather<29>(a, tot, part, ln, [](int) {}, [](int, int, int) {})) return;
    lm_solve_finish(a, lm, ln.seq, a.state[ln.seq], tot[threadIdx.x], a.ignore_active, ln.it_prev, ln.xi, ln.Tc);
}

// k_lm_begin: the entry table and the records at the start of a tracking call, one thread per sequence: lambda = lambda0, nothing
// accepted yet (the first evaluation of the coarsest level is FIRST and overwrites the rest), and "not tracked" until a solve says
// otherwise.
__global__ void __launch_bounds__(256) k_lm_begin(LmBeginArgs a)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_seq) return;
    dvo_lm_entry& e = a.table[i];
    e.lambda = a.lambda0; e.n_valid = 0; e.residual = -1.0f; e.reserved = 0;
    dvo_lm_record& r = a.last[i];
    r.n_first = 0; r.n_accepted = 0; r.n_rejected = 0; r.lambda = 0.0f; r.residual = 0.0f;
}

// k_lm_step: lm_solve_finish on given sums, one case per thread (dvo_op_lm_step): the state of xi_eval is set up as seed_state does.
__global__ void __launch_bounds__(64) k_lm_step(SolveArgs a, LmSolve lm, const double* __restrict__ sums, const float* __restrict__ xi_eval,
                                                int n, int it_prev)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    SeqState& st = a.state[i];
    float xi[6];
    double xd[6], Tc[12], tot[29];
    for (int k = 0; k < 6; k++) { xi[k] = xi_eval[6 * (size_t)i + k]; xd[k] = xi[k]; st.xi[k] = xi[k]; }
    pose_from_xi(xi, -1.0f, st.pose);
    se3_exp_d(xd, Tc, Tc + 9);
    for (int k = 0; k < 12; k++) st.Tc[k] = Tc[k];
    for (int k = 0; k < 29; k++) tot[k] = sums[29 * (size_t)i + k];
    lm_solve_finish(a, lm, i, st, tot, a.ignore_active, it_prev, xi, Tc);
}

// (the mapping kernels -- propagate, regularize, depth update, keyframe promotion -- live in dvo_map_kernels.hip)

// ------------------------------------------------------------------------------------------------
// Dataset front-end kernels (what src/core/loader.cpp does on the CPU with OpenCV)
// ------------------------------------------------------------------------------------------------
// k_ingest: raw sensor frames -> the float maps of the ABI, on the device (uploads 1.5 MB/frame instead of 3.7 MB).
//   gray  = BGR2GRAY(u8) / 255 (loader.cpp:55-60; OpenCV's fixed-point luma R 4899, G 9617, B 1868, >> 14), PNG channel
//           order is R,G,B[,A]; 1-channel input is taken as gray.
//   depth = u16 * depth_scale (loader.cpp:145: 1/5000), sigma = sigma_valid where depth > 0 else sigma_invalid and,
//   with invalidate_gray, gray = INVALID where depth == 0 -- what Transform::mapDepthtoGray leaves behind
//   (src/core/transform.cpp:60-76: pixels without depth stay INVALID with sigma 1, the others get sigma 0.1).
__global__ void __launch_bounds__(256) k_ingest(const uint8_t* __restrict__ rgb, int channels, const uint16_t* __restrict__ depth16,
                                                int n, float gray_scale, float depth_scale, float sigma_valid, float sigma_invalid,
                                                int invalidate_gray, float* __restrict__ gray, float* __restrict__ depth, float* __restrict__ sigma)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    unsigned g8;
    if (channels == 1) {
        g8 = rgb[i];
    } else {
        const uint8_t* p = rgb + (size_t)i * channels;
        g8 = ((unsigned)p[0] * 4899u + (unsigned)p[1] * 9617u + (unsigned)p[2] * 1868u + 8192u) >> 14;
    }
    float gv = (float)g8 * gray_scale;
    if (depth16) {
        const unsigned d = depth16[i];
        depth[i] = (float)d * depth_scale;
        sigma[i] = d > 0 ? sigma_valid : sigma_invalid;
        if (invalidate_gray && d == 0) gv = kInvalid;
    }
    gray[i] = gv;
}

// k_undistort: Loader::getNormalizedUndistortedImages (loader.cpp:15-42): cv::initUndistortRectifyMap(K, D, I, K) +
// cv::remap(INTER_NEAREST, BORDER_CONSTANT = INVALID), restated from the radial-tangential model definition.
__global__ void __launch_bounds__(256) k_undistort(const float* __restrict__ src, int w, int h, Intr k, float k1, float k2, float p1,
                                                   float p2, float k3, float border, float* __restrict__ dst)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= w * h) return;
    const int v = i / w, u = i - v * w;
    int si;
    float out = border;
    if (undistort_source(k, v, u, k1, k2, p1, p2, k3, w, h, si)) out = src[si];   // (dvo_math.h)
    dst[i] = out;
}

// k_undistort_map: the remap table of the undistortion fused into the mono pyramid (k_pyramid_remap), once per set_distortion.
// One thread per TOP-level pixel per distinct camera: the source index undistort_source gives full-resolution pixel
// (x << culls, y << culls), or -1.  Table [n_cam][th][tw]; grid seq_grid(., n_cam), the camera in place of the sequence.
__global__ void __launch_bounds__(256) k_undistort_map(const UndistortCam* __restrict__ cams, int n_cam, int w, int h, int culls, int tw,
                                                       int th, int* __restrict__ table)
{
    const int cam = (int)(blockIdx.z * DVO_GRID_SEQ_Y + blockIdx.y);
    const int i = (int)blockIdx.x * 256 + threadIdx.x;
    if (i >= tw * th || cam >= n_cam) return;
    const int y = i / tw, x = i - y * tw;
    const UndistortCam q = cams[cam];
    int si;
    if (!undistort_source(q.k, y << culls, x << culls, q.D[0], q.D[1], q.D[2], q.D[3], q.D[4], w, h, si)) si = -1;
    table[(size_t)cam * tw * th + i] = si;
}

// ------------------------------------------------------------------------------------------------
// k_visualize: the false-colour views of src/core/draw.cpp:7-100 as plain RGB bytes (no GUI).
//   mode 0 gray      (Draw::visualizeGray: value*255, INVALID pixels blue)
//   mode 1 depth     (Draw::visualizeDepth(depth, sigma): hue from depth, value from sigma; b may be null -> full value)
//   mode 2 sigma     (Draw::visualizeSigma: 255 - 500 sigma)
//   mode 3 age       (Draw::visualizeAge: 10 * age)
//   mode 4 gradient  (Draw::visualizeGradient: green positive, red negative, INVALID blue)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned char sat_u8(float v)
{
    v = rintf(v);
    return (unsigned char)(v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v));
}

__global__ void __launch_bounds__(256) k_visualize(int mode, const float* __restrict__ a, const float* __restrict__ b, int n, uint8_t* __restrict__ rgb)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = a[i];
    unsigned char R = 0, G = 0, B = 0;
    if (mode == 0) {
        R = G = B = sat_u8(v * 255.0f);
        if (!is_valid(v)) B = 255;
    } else if (mode == 1) {
        if (!(v < kEpsilon)) {
            const float hue = fminf(fmaxf((v - 0.70f) * 70.0f, 0.0f), 180.0f);  // OpenCV 8-bit hue: degrees / 2
            const float val = b ? (float)(unsigned char)(-500.0f * fminf(b[i], 0.5f) + 255.0f) / 255.0f : 1.0f;
            const float hh = (float)(unsigned char)hue * 2.0f / 60.0f;
            const float c = val, x = c * (1.0f - fabsf(fmodf(hh, 2.0f) - 1.0f));
            float r = 0, g = 0, bl = 0;
            if (hh < 1) { r = c; g = x; } else if (hh < 2) { r = x; g = c; } else if (hh < 3) { g = c; bl = x; }
            else if (hh < 4) { g = x; bl = c; } else if (hh < 5) { r = x; bl = c; } else { r = c; bl = x; }
            R = sat_u8(r * 255.0f); G = sat_u8(g * 255.0f); B = sat_u8(bl * 255.0f);
        }
    } else if (mode == 2) {
        R = G = B = sat_u8(v * -500.0f + 255.0f);
    } else if (mode == 3) {
        R = G = B = sat_u8(v * 10.0f);
    } else {
        if (is_invalid(v)) B = 255;
        else { G = (unsigned char)(255.0f * fminf(fmaxf(v, 0.0f), 1.0f)); R = (unsigned char)(255.0f * fminf(fmaxf(-v, 0.0f), 1.0f)); }
    }
    rgb[3 * (size_t)i] = R; rgb[3 * (size_t)i + 1] = G; rgb[3 * (size_t)i + 2] = B;
}

// ------------------------------------------------------------------------------------------------
// launch wrappers (host)
// ------------------------------------------------------------------------------------------------
// k_selftest_reciprocal: recip_rn() (dvo_math.h) against the IEEE division for ALL 2^32 float bit patterns.
// out[0] = patterns that took the rcp + 2 FMA branch, out[1] = mismatching patterns (must be 0), out[2] = smallest bad pattern.
__global__ void __launch_bounds__(256) k_selftest_reciprocal(unsigned long long* out)
{
    unsigned long long fast = 0, bad = 0, first = ~0ull;
    for (unsigned long long p = blockIdx.x * 256ull + threadIdx.x; p < (1ull << 32); p += (unsigned long long)gridDim.x * 256ull) {
        const float z = __uint_as_float((unsigned)p);
        const float az = fabsf(z);
        const float want = 1.0f / z, got = recip_rn(z);
        const bool same = (__float_as_uint(got) == __float_as_uint(want)) || (got != got && want != want);
        if (az >= DVO_RECIP_FAST_MIN && az <= DVO_RECIP_FAST_MAX) fast++;
        if (!same) { bad++; if (p < first) first = p; }
    }
    atomicAdd(&out[0], fast);
    atomicAdd(&out[1], bad);
    atomicMin(&out[2], first);
}

// k_selftest_sqrt: sqrt_fast() (dvo_math.h; the regularize kernels' square root) against sqrtf for every float in [2^-100, 2^100].
// k_selftest_division: div_by_recip(a, b, recip_fast(b)) against a / b for b = 1.mb, mb = b_first + i * b_stride (i < b_count), and ALL
// 2^23 mantissas of a in [1, 2) -- the operations after v_rcp_f32 (whose every input recip_fast() was enumerated on:
// k_selftest_reciprocal) are IEEE multiplies and FMAs, scale invariant inside the normal range, so mantissa pairs are all there is to check.
// out = {operands checked, mismatches, first bad (sqrt: bit pattern; division: mb << 23 | ma)}, pre-set {0, 0, ~0}.
__global__ void __launch_bounds__(256) k_selftest_sqrt(unsigned long long* out)
{
    unsigned long long n = 0, bad = 0, first = ~0ull;
    for (unsigned long long p = blockIdx.x * 256ull + threadIdx.x; p < (1ull << 31); p += (unsigned long long)gridDim.x * 256ull) {
        const float x = __uint_as_float((unsigned)p);
        if (!(x >= DVO_RECIP_FAST_MIN && x <= DVO_RECIP_FAST_MAX)) continue;
        n++;
        if (__float_as_uint(sqrt_fast(x)) != __float_as_uint(sqrtf(x))) { bad++; if (p < first) first = p; }
    }
    atomicAdd(&out[0], n);
    if (bad) { atomicAdd(&out[1], bad); atomicMin(&out[2], first); }
}

__global__ void __launch_bounds__(256) k_selftest_division(unsigned b_first, unsigned b_stride, unsigned b_count, unsigned long long* out)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= b_count) return;
    const unsigned mb = (b_first + i * b_stride) & 0x7fffffu;
    const float b = __uint_as_float(0x3f800000u | mb);
    const float y = recip_fast(b);
    unsigned long long bad = 0, first = ~0ull;
    for (unsigned ma = 0; ma < (1u << 23); ma++) {
        const float a = __uint_as_float(0x3f800000u | ma);
        if (__float_as_uint(div_by_recip(a, b, y)) != __float_as_uint(a / b)) { bad++; const unsigned long long k = ((unsigned long long)mb << 23) | ma; if (k < first) first = k; }
    }
    atomicAdd(&out[0], 1ull << 23);
    if (bad) { atomicAdd(&out[1], bad); atomicMin(&out[2], first); }
}

// k_selftest_trig: the SE(3) chain's sin / cos / atan2 (dvo_math.h: sincos_dev, atan2_dev) against the math library over their domain:
// sample i of n -> x log-spaced in [1e-12, 1e5) (even i) or uniform in [0, 16) (odd i) for sin / cos; (s, c) = (u, 2v - 1), u in (0, 1],
// v in [0, 1] on a sqrt(n) x sqrt(n) grid plus the same scaled by 1e-9 for atan2 (the log map feeds it sqrt(...) and a trace).
// out[0..2] = largest relative difference (as the bits of a non-negative double) of sin, cos, atan2.
__global__ void __launch_bounds__(256) k_selftest_trig(unsigned n, unsigned side, unsigned long long* out)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const double f = ((double)i + 0.5) / (double)n;
    const double x = (i & 1) ? 16.0 * f : exp(log(1e-12) + f * (log(1e5) - log(1e-12)));
    double sd, cd;
    sincos_dev(x, sd, cd);
    const double sl = sin(x), cl = cos(x);
    const double es = fabs(sd - sl) / fabs(sl), ec = fabs(cd - cl) / fabs(cl);
    const unsigned gy = i / side, gx = i - gy * side;
    double y = ((double)gy + 1.0) / (double)side, c = 2.0 * ((double)gx / (double)(side - 1)) - 1.0;
    if (gy & 1) { y *= 1e-9; }
    const double ad = atan2_dev(y, c), al = atan2(y, c);
    const double ea = fabs(ad - al) / fabs(al);
    atomicMax(&out[0], (unsigned long long)__double_as_longlong(es));
    atomicMax(&out[1], (unsigned long long)__double_as_longlong(ec));
    atomicMax(&out[2], (unsigned long long)__double_as_longlong(ea));
}
void launch_selftest_trig(unsigned n, unsigned side, unsigned long long* out, hipStream_t s)
{
    hipLaunchKernelGGL(k_selftest_trig, dim3((n + 255) / 256), dim3(256), 0, s, n, side, out);
}

void launch_selftest_sqrt(unsigned long long* out, hipStream_t s) { hipLaunchKernelGGL(k_selftest_sqrt, dim3(8192), dim3(256), 0, s, out); }
void launch_selftest_division(unsigned b_first, unsigned b_stride, unsigned b_count, unsigned long long* out, hipStream_t s)
{
    hipLaunchKernelGGL(k_selftest_division, dim3((b_count + 255) / 256), dim3(256), 0, s, b_first, b_stride, b_count, out);
}

void launch_selftest_reciprocal(unsigned long long* out, hipStream_t s)
{
    hipLaunchKernelGGL(k_selftest_reciprocal, dim3(8192), dim3(256), 0, s, out);
}

void launch_visualize(int mode, const float* a, const float* b, int n, uint8_t* rgb, hipStream_t s)
{
    hipLaunchKernelGGL(k_visualize, dim3((n + 255) / 256), dim3(256), 0, s, mode, a, b, n, rgb);
}

void launch_ingest(const uint8_t* rgb, int channels, const uint16_t* depth16, int n, float depth_scale, float sigma_valid,
                   float sigma_invalid, int invalidate_gray, float* gray, float* depth, float* sigma, hipStream_t s)
{
    hipLaunchKernelGGL(k_ingest, dim3((n + 255) / 256), dim3(256), 0, s, rgb, channels, depth16, n, (float)(1.0 / 255.0), depth_scale,
                       sigma_valid, sigma_invalid, invalidate_gray, gray, depth, sigma);
}

void launch_undistort(const float* src, int w, int h, const Intr& k, const float D[5], float border, float* dst, hipStream_t s)
{
    hipLaunchKernelGGL(k_undistort, dim3((w * h + 255) / 256), dim3(256), 0, s, src, w, h, k, D[0], D[1], D[2], D[3], D[4], border, dst);
}

static inline unsigned cdiv(unsigned a, unsigned b) { return (a + b - 1) / b; }

void launch_undistort_map(const UndistortCam* cams_dev, int n_cam, int w, int h, int culls, int tw, int th, int* table, hipStream_t s)
{
    hipLaunchKernelGGL(k_undistort_map, seq_grid(cdiv(tw * th, 256), (unsigned)n_cam), dim3(256), 0, s, cams_dev, n_cam, w, h, culls, tw, th, table);
}

void launch_photometric_map(const float* vignette, const int* pairs, int n_pair, int w, int h, int culls, int tw, int th, const int* remap,
                            float* gain, hipStream_t s)
{
    hipLaunchKernelGGL(k_photometric_map, seq_grid(cdiv(tw * th, 256), (unsigned)n_pair), dim3(256), 0, s, vignette, pairs, n_pair, w, h, culls,
                       tw, th, remap, gain);
}

// A runtime flag as a compile-time constant: f receives std::true_type or std::false_type, so a launcher names its kernel template
// once and the flag's two instances follow from it
template <class F>
static void with_flag(bool on, F&& f)
{
    if (on) f(std::true_type{});
    else f(std::false_type{});
}

// The CULLS of the four-pixel pyramid kernels (1 or 2, pyramid_raw4_possible) as a compile-time constant, like with_flag
template <class F>
static void with_culls(int culls, F&& f)
{
    if (culls == 1) f(std::integral_constant<int, 1>{});
    else f(std::integral_constant<int, 2>{});
}

// Every pointer is 16-byte aligned (nullptr passes: not accessed)
static bool aligned16(std::initializer_list<const void*> ptrs)
{
    for (const void* p : ptrs)
        if ((reinterpret_cast<uintptr_t>(p) % 16) != 0) return false;
    return true;
}

// The grid of a pyramid kernel whose threads own ppt consecutive pixels of a w x h level (ppt = 4: w is a multiple of 4)
static dim3 pyramid_grid(int w, int h, int ppt, int n_seq) { return seq_grid(cdiv((w / ppt) * h, 256), (unsigned)n_seq); }

// The four-pixel build (k_pyramid_raw4, _photo, _rest) is possible for these arguments: 1-channel bytes, CULLS 1 or 2, whole
// groups of four kept pixels in whole 16-byte source words, and 16-byte aligned input and top-level maps; `more` are the
// caller's kernel's further 16-byte accesses.
static bool pyramid_raw4_possible(const PyramidArgs& a, std::initializer_list<const void*> more)
{
    const int T = a.levels - 1, tw = a.w[T], th = a.h[T];
    return a.raw_rgb != nullptr && a.raw_channels == 1 && (a.culls == 1 || a.culls == 2) && (tw % 4) == 0 && (a.src_w % (4 << a.culls)) == 0 &&
           ((size_t)tw * th % 4) == 0 && aligned16({a.raw_rgb, a.raw_depth, a.dst[0][T], a.dst[1][T], a.dst[2][T], a.wgt[T]}) && aligned16(more);
}

// k_pyramid_remap_depth: four kept pixels per thread where the top-level width and every 16-byte access allow it, else one
// (DVO_REMAP_DEPTH_SCALAR set: always one -- A/B runs, tools/bench_sensor_undistort.py)
static void launch_pyramid_remap_depth(const PyramidArgs& a, hipStream_t s)
{
    const int T = a.levels - 1, tw = a.w[T], th = a.h[T];
    const bool vec = (tw % 4) == 0 && getenv("DVO_REMAP_DEPTH_SCALAR") == nullptr &&
                     aligned16({a.remap, a.dst[0][T], a.dst[1][T], a.dst[2][T], a.wgt[T], a.ref[0][T], a.ref[1][T], a.ref[2][T], a.ref_wgt[T]});
    with_flag(a.seq_action != nullptr, [&](auto plan) {
        constexpr bool PLAN = decltype(plan)::value;
        if (vec) hipLaunchKernelGGL((k_pyramid_remap_depth<4, PLAN>), pyramid_grid(tw, th, 4, a.n_seq), dim3(256), 0, s, a);
        else hipLaunchKernelGGL((k_pyramid_remap_depth<1, PLAN>), pyramid_grid(tw, th, 1, a.n_seq), dim3(256), 0, s, a);
    });
}

// The kernels of a calibrated handle's raw mono frames (PhotoArgs set): k_pyramid_raw4_photo where the four-pixel build is possible
// at culls 2 with 16-byte gain rows, else k_pyramid_photo.  A missing piece is an error of the caller (build_pyramid checks), not a
// reason to run a plain kernel.
static PyramidKernel launch_pyramid_photo(const PyramidArgs& a, const PhotoArgs& p, hipStream_t s)
{
    const int T = a.levels - 1, tw = a.w[T], th = a.h[T];
    const bool plan = a.seq_action != nullptr, remap = a.remap != nullptr;
    PyramidKernel ran = {remap ? DVO_PYRAMID_KERNEL_PHOTO_REMAP : DVO_PYRAMID_KERNEL_PHOTO_SCALAR, 0, plan ? 1 : 0};
    with_flag(plan, [&](auto plan_c) {
        constexpr bool PLAN = decltype(plan_c)::value;
        if (!remap && a.culls == 2 && pyramid_raw4_possible(a, {p.gain, PLAN ? a.ref[0][T] : nullptr})) {
            const char* e = getenv("DVO_PHOTO_RESPONSE");
            with_flag(!(e && strcmp(e, "global") == 0), [&](auto lds) {
                hipLaunchKernelGGL((k_pyramid_raw4_photo<2, PLAN, decltype(lds)::value>), pyramid_grid(tw, th, 4, a.n_seq), dim3(256), 0, s, a, p);
            });
            ran = {DVO_PYRAMID_KERNEL_PHOTO_RAW4, a.culls, plan ? 1 : 0};
            return;
        }
        with_flag(remap, [&](auto remap_c) {
            hipLaunchKernelGGL((k_pyramid_photo<PLAN, decltype(remap_c)::value>), pyramid_grid(tw, th, 1, a.n_seq), dim3(256), 0, s, a, p);
        });
    });
    return ran;
}

// k_pyramid_filter_top's 16-byte staging loads are possible: whole chunks (16 one-channel bytes with their two depth words, or 4
// floats) per row and 16-byte aligned inputs.  The level maps are stored one float at a time, so their alignment (a batch whose
// size is no multiple of 4) does not matter here.
static bool pyramid_filter_wide(const PyramidArgs& a)
{
    if (a.culls < 1 || getenv("DVO_PYRAMID_FILTER_SCALAR") != nullptr) return false;   // (the variable: A/B runs, tests)
    if (a.raw_rgb != nullptr) return a.raw_channels == 1 && (a.src_w % 16) == 0 && aligned16({a.raw_rgb, a.raw_depth});
    return (a.src_w % 4) == 0 && aligned16({a.src[0]});
}

// The binomial-filtered build: k_pyramid_filter_top on 32 x 8 tiles of the top level, then one
// k_pyramid_filter_down per level below it.  PyramidKernel::plan carries the instance: bit 0 PLAN, bit 1 WIDE, bit 2 RAW.
static PyramidKernel launch_pyramid_filter(const PyramidArgs& a, hipStream_t s)
{
    const int T = a.levels - 1, tw = a.w[T], th = a.h[T];
    const bool plan = a.seq_action != nullptr, raw = a.raw_rgb != nullptr, wide = pyramid_filter_wide(a);
    const dim3 grid = seq_grid(cdiv(tw, 32) * cdiv(th, 8), (unsigned)a.n_seq);
    with_flag(plan, [&](auto plan_c) {
        with_flag(raw, [&](auto raw_c) {
            constexpr bool PLAN = decltype(plan_c)::value, RAW = decltype(raw_c)::value;
            if (a.culls == 0) {
                hipLaunchKernelGGL((k_pyramid_filter_top<0, RAW, PLAN, false>), grid, dim3(256), 0, s, a);
                return;
            }
            with_culls(a.culls, [&](auto culls) {
                with_flag(wide, [&](auto wide_c) {
                    hipLaunchKernelGGL((k_pyramid_filter_top<decltype(culls)::value, RAW, PLAN, decltype(wide_c)::value>), grid, dim3(256), 0, s, a);
                });
            });
        });
        for (int l = T - 1; l >= 0; l--)
            hipLaunchKernelGGL(k_pyramid_filter_down<decltype(plan_c)::value>, pyramid_grid(a.w[l], a.h[l], 1, a.n_seq), dim3(256), 0, s, a, l,
                               1.0f / (float)a.w[l]);
    });
    return {DVO_PYRAMID_KERNEL_FILTER, a.culls, (plan ? 1 : 0) | (wide ? 2 : 0) | (raw ? 4 : 0)};
}

PyramidKernel launch_pyramid(const PyramidArgs& a0, int n_seq, hipStream_t s, const PhotoArgs* photo, int filter)
{
    PyramidArgs a = a0;
    a.n_seq = n_seq;
    if (filter != DVO_PYRAMID_FILTER_NONE) return launch_pyramid_filter(a, s);   // (the callers refuse it with a photo block or a remap)
    if (photo != nullptr && photo->gain != nullptr) return launch_pyramid_photo(a, *photo, s);
    const int T = a.levels - 1, tw = a.w[T], th = a.h[T];
    const bool plan = a.seq_action != nullptr;
    if (a.remap != nullptr) {   // lens undistortion fused in: never k_pyramid_raw4 / k_pyramid
        if (a.raw_depth != nullptr || a.src[1] != nullptr) launch_pyramid_remap_depth(a, s);   // sensor-depth frames
        else if (plan) hipLaunchKernelGGL(k_pyramid_remap_plan, pyramid_grid(tw, th, 1, n_seq), dim3(256), 0, s, a);   // mono frames
        else hipLaunchKernelGGL(k_pyramid_remap, pyramid_grid(tw, th, 1, n_seq), dim3(256), 0, s, a);
        return {DVO_PYRAMID_KERNEL_REMAP, 0, plan ? 1 : 0};
    }
    PyramidKernel ran = {DVO_PYRAMID_KERNEL_SCALAR, 0, plan ? 1 : 0};
    with_flag(plan, [&](auto plan_c) {
        constexpr bool PLAN = decltype(plan_c)::value;
        // raw 1-channel frames with the usual alignment: four kept pixels per thread, wide loads and stores (with a plan the
        // copy-forward reads the reference tops with the same 16-byte accesses)
        if (PLAN ? pyramid_raw4_possible(a, {a.ref[0][T], a.ref[1][T], a.ref[2][T], a.ref_wgt[T]}) : pyramid_raw4_possible(a, {})) {
            with_culls(a.culls, [&](auto culls) {
                hipLaunchKernelGGL((k_pyramid_raw4<decltype(culls)::value, PLAN>), pyramid_grid(tw, th, 4, n_seq), dim3(256), 0, s, a);
            });
            ran = {DVO_PYRAMID_KERNEL_RAW4, a.culls, plan ? 1 : 0};
            return;
        }
        hipLaunchKernelGGL(k_pyramid<PLAN>, pyramid_grid(tw, th, 1, n_seq), dim3(256), 0, s, a);
    });
    return ran;
}

bool pyramid_can_split(const PyramidArgs& a)
{
    const int T = a.levels - 1;
    if (a.levels < 2 || a.remap != nullptr || a.seq_action != nullptr || a.raw_depth == nullptr) return false;
    // stage B: the four-pixel build; stage A: eight top-level pixels per thread, a dwordx4 store into level top - 1
    if (!pyramid_raw4_possible(a, {a.dst[0][T - 1]})) return false;
    const int tw = a.w[T], th = a.h[T];
    return (tw % 8) == 0 && (a.src_w % (8 << a.culls)) == 0 && ((size_t)a.w[T - 1] * a.h[T - 1] % 4) == 0 && a.w[T - 1] * 2 == tw && a.h[T - 1] * 2 <= th;
}

void launch_pyramid_coarse(const PyramidArgs& a0, int n_seq, hipStream_t s)
{
    PyramidArgs a = a0;
    a.n_seq = n_seq;
    const int T = a.levels - 1;
    with_culls(a.culls, [&](auto culls) {
        hipLaunchKernelGGL(k_pyramid_raw4_coarse<decltype(culls)::value>, pyramid_grid(a.w[T - 1], a.h[T - 1], 4, n_seq), dim3(256), 0, s, a);
    });
}

void launch_pyramid_rest(const PyramidArgs& a0, int n_seq, hipStream_t s)
{
    PyramidArgs a = a0;
    a.n_seq = n_seq;
    const int T = a.levels - 1;
    with_culls(a.culls, [&](auto culls) {
        hipLaunchKernelGGL(k_pyramid_raw4_rest<decltype(culls)::value>, pyramid_grid(a.w[T], a.h[T], 4, n_seq), dim3(256), 0, s, a);
    });
}

void launch_cull(const float* src, int w, int h, int times, float* dst, hipStream_t s)
{
    const int n = (w >> times) * (h >> times);
    hipLaunchKernelGGL(k_cull, dim3(cdiv(n, 256)), dim3(256), 0, s, src, w, h, times, dst);
}

void launch_gradient(const float* img, int w, int h, int xdir, float* out, hipStream_t s)
{
    hipLaunchKernelGGL(k_gradient, dim3(cdiv(w * h, 256)), dim3(256), 0, s, img, w, h, xdir, out);
}

void launch_warp_image(const float* gray, const float* depth, int w, int h, const Intr& k, const Pose& pose, float* out, hipStream_t s)
{
    hipLaunchKernelGGL(k_warp_image, dim3(cdiv(w * h, 256)), dim3(256), 0, s, gray, depth, w, h, k, pose, out);
}

int gn_blocks_per_seq(int w, int h, int ppt, int crop) { return gn_tiling(w, h, ppt, crop).count; }

// The (ppt, group) pairs the tilings pick, as compile-time constants: f receives the pair as two std::integral_constant, so a launcher
// names its kernel template once and the nine instances follow from it.  Any other pair runs as <8, 4>.
template <class F>
static void with_gn_shape(int ppt, int group, F&& f)
{
    using std::integral_constant;
    switch (ppt * 10 + group) {
        case 11: f(integral_constant<int, 1>{}, integral_constant<int, 1>{}); break;
        case 21: f(integral_constant<int, 2>{}, integral_constant<int, 1>{}); break;
        case 22: f(integral_constant<int, 2>{}, integral_constant<int, 2>{}); break;
        case 41: f(integral_constant<int, 4>{}, integral_constant<int, 1>{}); break;
        case 42: f(integral_constant<int, 4>{}, integral_constant<int, 2>{}); break;
        case 44: f(integral_constant<int, 4>{}, integral_constant<int, 4>{}); break;
        case 81: f(integral_constant<int, 8>{}, integral_constant<int, 1>{}); break;
        case 82: f(integral_constant<int, 8>{}, integral_constant<int, 2>{}); break;
        default: f(integral_constant<int, 8>{}, integral_constant<int, 4>{}); break;
    }
}

// The grid of a tile launch (k_track_gn and the opt-in tile kernels), a multiple of 8: blockIdx % 8 is the XCD.
// grid_seqs: an upper bound of the sequences on the active list (the host knows one from the progress words): the grid then only
// holds workgroups that can find a tile -- at 16 384 sequences x 75 tiles an all-empty grid alone costs ~0.35 ms to dispatch
static dim3 gn_tile_grid(const GnArgs& a, int n_seq, int grid_seqs)
{
    const int gs = (grid_seqs > 0 && grid_seqs < n_seq && a.list != nullptr) ? grid_seqs : n_seq;
    unsigned tiles = (unsigned)a.blk_count * (unsigned)gs;
    if (tiles == 0) tiles = 8;  // (nothing live: the workgroups only clear the next list counter)
    return dim3((tiles + 7u) & ~7u);
}

void launch_track_gn(const GnArgs& a0, int n_seq, int ppt, int group, bool t2d, hipStream_t s, int grid_seqs)
{
    GnArgs a = a0;
    a.n_seq = n_seq;
    const dim3 grid = gn_tile_grid(a, n_seq, grid_seqs);
    with_gn_shape(ppt, group, [&](auto p, auto g) {
        constexpr int PPT = decltype(p)::value, G = decltype(g)::value;
        with_flag(a.mask != nullptr, [&](auto mask) {
            with_flag(PPT == 4 && t2d, [&](auto tiles_2d) {   // (2-D tiles exist for 4 pixels per thread only)
                constexpr bool MASK = decltype(mask)::value, T2D = PPT == 4 && decltype(tiles_2d)::value;
                if (a.seq_k) hipLaunchKernelGGL((k_track_gn_cam<PPT, G, MASK, T2D>), grid, dim3(256), 0, s, a);   // per-sequence intrinsics
                else hipLaunchKernelGGL((k_track_gn<PPT, G, MASK, T2D>), grid, dim3(256), 0, s, a);
            });
        });
    });
}

// One tile launch of an opt-in term.  pair(p, g, tiles_2d, cam) is the term's kernel instance for the (ppt, group) pair, the 2-D tiles
// flag (PPT = 4 only) and the per-sequence intrinsics (_cam); blocks: the term's argument blocks, forwarded behind GnArgs.
// (the opt-in tile kernels have no MASK instances: a.mask = nullptr)
template <class Pair, class... Blocks>
static void launch_term_tiles(const GnArgs& a0, int n_seq, int ppt, int group, bool t2d, hipStream_t s, int grid_seqs, Pair&& pair,
                              const Blocks&... blocks)
{
    GnArgs a = a0;
    a.n_seq = n_seq; a.mask = nullptr;
    const dim3 grid = gn_tile_grid(a, n_seq, grid_seqs);
    with_gn_shape(ppt, group, [&](auto p, auto g) {
        constexpr int PPT = decltype(p)::value;
        with_flag(PPT == 4 && t2d, [&](auto tiles_2d) {
            constexpr std::bool_constant<PPT == 4 && decltype(tiles_2d)::value> t2d_c{};
            hipLaunchKernelGGL(pair(p, g, t2d_c, a.seq_k != nullptr), grid, dim3(256), 0, s, a, blocks...);
        });
    });
}

// The table "set of terms -> tile kernel pair" (the solve side's is launch_gn_solve_terms)
bool launch_track_gn_terms(const GnArgs& a, const TileTerms& t, int n_seq, int ppt, int group, bool t2d, hipStream_t s, int grid_seqs)
{
    const auto tiles = [&](auto&& pair, const auto&... blocks) {
        launch_term_tiles(a, n_seq, ppt, group, t2d, s, grid_seqs, pair, blocks...);
        return true;
    };
    // (a pair: the instance of a term's kernel and of its _cam twin, from the constants with_gn_shape and with_flag pass)
    switch (t.on) {
    case 0:
    case TERM_STEP_CONTROL: launch_track_gn(a, n_seq, ppt, group, t2d, s, grid_seqs); return true;   // (only the solve differs)
    case TERM_ROBUST:
        return tiles([](auto p, auto g, auto t2, bool cam) {
            constexpr int P = p, G = g; constexpr bool T = t2;
            return cam ? k_track_gn_rw_cam<P, G, T> : k_track_gn_rw<P, G, T>;
        }, t.rob);
    case TERM_MEDIAN:
        return tiles([](auto p, auto g, auto t2, bool cam) {
            constexpr int P = p, G = g; constexpr bool T = t2;
            return cam ? k_track_gn_md_cam<P, G, T> : k_track_gn_md<P, G, T>;
        }, t.rob, t.med);
    case TERM_AFFINE:
    case TERM_ROBUST | TERM_AFFINE:
        with_flag(t.rob.table != nullptr, [&](auto robust) {
            tiles([](auto p, auto g, auto t2, bool cam) {
                constexpr int P = p, G = g; constexpr bool T = t2, ROB = decltype(robust)::value;
                return cam ? k_track_gn_ab_cam<P, G, T, ROB> : k_track_gn_ab<P, G, T, ROB>;
            }, t.rob, t.aff);
        });
        return true;
    case TERM_GEOMETRIC:
        return tiles([](auto p, auto g, auto t2, bool cam) {
            constexpr int P = p, G = g; constexpr bool T = t2;
            return cam ? k_track_gn_z_cam<P, G, T> : k_track_gn_z<P, G, T>;
        }, t.geo);
    case TERM_GEOMETRIC | TERM_AFFINE:
        return tiles([](auto p, auto g, auto t2, bool cam) {
            constexpr int P = p, G = g; constexpr bool T = t2;
            return cam ? k_track_gn_zab_cam<P, G, T> : k_track_gn_zab<P, G, T>;
        }, t.aff, t.geo);
    default: return false;
    }
}

// A solve kernel (k_gn_solve or an opt-in term's) over n_seq sequences, DVO_SOLVE_SEQ per workgroup; extra: the term's argument blocks
template <class K, class... Extra>
static void launch_solve_kernel(K kernel, const SolveArgs& a, int n_seq, hipStream_t s, const Extra&... extra)
{
    SolveArgs b = a;
    b.n_seq = n_seq;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n_seq + DVO_SOLVE_SEQ - 1) / DVO_SOLVE_SEQ)), dim3(32 * DVO_SOLVE_SEQ), 0, s, b, extra...);
}

void launch_gn_solve(const SolveArgs& a, int n_seq, hipStream_t s) { launch_solve_kernel(k_gn_solve, a, n_seq, s); }

// The table "set of terms -> solve kernel" (launch_track_gn_terms's partner)
bool launch_gn_solve_terms(const SolveArgs& a, const SolveTerms& t, int n_seq, hipStream_t s)
{
    switch (t.on) {
    case 0: launch_solve_kernel(k_gn_solve, a, n_seq, s); return true;
    case TERM_ROBUST: launch_solve_kernel(k_gn_solve_rw, a, n_seq, s, t.rob); return true;
    case TERM_MEDIAN: launch_solve_kernel(k_gn_solve_md, a, n_seq, s, t.rob, t.med); return true;
    case TERM_AFFINE:
    case TERM_ROBUST | TERM_AFFINE: launch_solve_kernel(k_gn_solve_ab, a, n_seq, s, t.rob, t.aff); return true;
    case TERM_GEOMETRIC: launch_solve_kernel(k_gn_solve_z, a, n_seq, s, t.geo); return true;
    case TERM_GEOMETRIC | TERM_AFFINE: launch_solve_kernel(k_gn_solve_zab, a, n_seq, s, t.aff, t.geo); return true;
    case TERM_STEP_CONTROL: launch_solve_kernel(k_gn_solve_lm, a, n_seq, s, t.lm); return true;
    default: return false;
    }
}

void launch_median_begin(const MedianBeginArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_median_begin, dim3((unsigned)a.n_seq), dim3(DVO_MEDIAN_BINS), 0, s, a);
}

void launch_robust_begin(const RobustBeginArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_robust_begin, dim3(cdiv(a.n_seq, 256)), dim3(256), 0, s, a);
}

void launch_lm_begin(const LmBeginArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_lm_begin, dim3(cdiv(a.n_seq, 256)), dim3(256), 0, s, a);
}

void launch_lm_step(const SolveArgs& a, const LmSolve& m, const double* sums, const float* xi_eval, int n, int it_prev, hipStream_t s)
{
    hipLaunchKernelGGL(k_lm_step, dim3(cdiv(n, 64)), dim3(64), 0, s, a, m, sums, xi_eval, n, it_prev);
}

void launch_affine_begin(const AffineBeginArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_affine_begin, dim3(cdiv(a.n_seq, 256)), dim3(256), 0, s, a);
}

// The (ppt, group) pairs the tiling picks for a handle of a few sequences: the ones k_track_gn_fused and k_track_persist have an
// instance for.  f receives the pair as with_gn_shape passes it; false (f not called) for any other pair.
template <class F>
static bool with_small_handle_pair(int ppt, int group, F&& f)
{
    bool found = false;
    with_gn_shape(ppt, group, [&](auto p, auto g) {
        constexpr int pair = decltype(p)::value * 10 + decltype(g)::value;
        if constexpr (pair == 11 || pair == 22 || pair == 42) {   // (no instance of f for the other six)
            f(p, g);
            found = true;
        }
    });
    return found;
}

bool gn_fused_available(int ppt, int group) { return with_small_handle_pair(ppt, group, [](auto, auto) {}); }
bool track_persist_available(int ppt, int group) { return gn_fused_available(ppt, group); }

// k_track_gn_fused for the (ppt, group) pairs the small-batch tiling picks; returns false when there is no such instance
bool launch_track_gn_fused(const GnArgs& a0, const SolveArgs& sa0, int n_seq, int ppt, int group, bool t2d, int* ticket, int* report,
                           int* progress, hipStream_t s)
{
    GnArgs a = a0;
    SolveArgs sa = sa0;
    a.n_seq = n_seq; a.list = nullptr; a.next_count = nullptr; a.mask = nullptr;
    sa.n_seq = n_seq; sa.list_in = nullptr; sa.list_out = nullptr; sa.progress = nullptr;
    if (a.blk_count <= 0) return false;
    FusedArgs f{ticket, report, progress, n_seq};
    const dim3 grid((unsigned)a.blk_count * (unsigned)n_seq);
    return with_small_handle_pair(ppt, group, [&](auto p, auto g) {
        with_flag(a.seq_k != nullptr, [&](auto cam) {   // per-sequence intrinsics
            with_flag(p.value == 4 && t2d, [&](auto tiles_2d) {
                constexpr int PPT = decltype(p)::value, G = decltype(g)::value;
                constexpr bool T2D = PPT == 4 && decltype(tiles_2d)::value, PCAM = decltype(cam)::value;
                hipLaunchKernelGGL((k_track_gn_fused<PPT, G, T2D, PCAM>), grid, dim3(256), 0, s, a, sa, f);
            });
        });
    });
}

// (k_track_persist's gather group only sets how many pixels' gathers are in flight together, never a result: the kernel runs one wave
//  per SIMD whatever it does, so it takes all of a thread's pixels at once -- the instance of a pair is <ppt, ppt>)
int track_persist_max_grid(int ppt, int group, int* out)
{
    int per_cu = 0, dev = 0;
    hipError_t e = hipErrorInvalidValue;
    with_small_handle_pair(ppt, group, [&](auto p, auto) {
        constexpr int PPT = decltype(p)::value;
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_track_persist<PPT, PPT, true>, 256, 0);   // (the instance with more registers)
    });
    if (e != hipSuccess) return DVO_ERR_HIP;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return DVO_ERR_HIP;
    *out = per_cu * prop.multiProcessorCount;
    return DVO_OK;
}

bool launch_track_persist(const PersistArgs& p, int ppt, int group, int grid, hipStream_t s)
{
    if (grid < 1) return false;
    return with_small_handle_pair(ppt, group, [&](auto pp, auto) {
        with_flag(p.mono.enabled != 0, [&](auto mono) {
            constexpr int PPT = decltype(pp)::value;
            hipLaunchKernelGGL((k_track_persist<PPT, PPT, decltype(mono)::value>), dim3(grid), dim3(256), 0, s, p);
        });
    });
}

void launch_track_level(const GnArgs& ga0, const SolveArgs& sa0, int n_seq, hipStream_t s)
{
    GnArgs ga = ga0;   // (raster tiles of 4 pixels per thread: Tracker::init fuses no other level)
    SolveArgs sa = sa0;
    ga.n_seq = n_seq;
    ga.list = nullptr; ga.next_count = nullptr; ga.mask = nullptr;
    sa.list_in = nullptr; sa.list_out = nullptr;
    with_flag(ga.seq_k != nullptr, [&](auto cam) {
        hipLaunchKernelGGL((k_track_level<4, 2, decltype(cam)::value>), dim3((unsigned)n_seq), dim3(256), 0, s, ga, sa);
    });
}

template <int PPT>
static void launch_track_gn_tile_t(const GnArgs& a, const dim3& grid, hipStream_t s)
{
    const size_t lds = (128 + (size_t)(4 * PPT + 2 * a.margin + 3) * (64 + 2 * a.margin + 3)) * sizeof(float);
    with_flag(a.mask != nullptr, [&](auto mask) {
        with_flag(a.seq_k != nullptr, [&](auto cam) {   // per-sequence intrinsics
            hipLaunchKernelGGL((k_track_gn_tile<PPT, decltype(mask)::value, decltype(cam)::value>), grid, dim3(256), lds, s, a);
        });
    });
}

void launch_track_gn_tile(const GnArgs& a, int n_seq, int ppt, hipStream_t s)
{
    const dim3 grid((unsigned)a.nblk * (unsigned)n_seq);
    switch (ppt) {
        case 1: launch_track_gn_tile_t<1>(a, grid, s); break;
        case 2: launch_track_gn_tile_t<2>(a, grid, s); break;
        case 4: launch_track_gn_tile_t<4>(a, grid, s); break;
        default: launch_track_gn_tile_t<8>(a, grid, s); break;
    }
}

void launch_prep_ref(const PrepArgs& a, hipStream_t s)
{
    const size_t n = a.level_end[a.levels - 1];
    if (n == 0) return;
    hipLaunchKernelGGL(k_prep_ref, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
}

void launch_track_begin(SeqState* state, dvo_track_log* log, int n_seq, int levels, hipStream_t s)
{
    hipLaunchKernelGGL(k_track_begin, dim3(cdiv(n_seq, 256)), dim3(256), 0, s, state, log, n_seq, levels);
}

void launch_plan(const PlanArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_plan, dim3(cdiv((unsigned)a.n_seq, 256)), dim3(256), 0, s, a);
}

void launch_set_pose(SeqState* state, const float* xi_dev, int n_seq, hipStream_t s)
{
    hipLaunchKernelGGL(k_set_pose, dim3(cdiv(n_seq, 64)), dim3(64), 0, s, state, xi_dev, n_seq);
}

void launch_seed_pose(const PoseSeedArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_seed_pose, dim3(cdiv(a.n_seq, 256)), dim3(256), 0, s, a);
}

void launch_track_quality(const QualityArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_track_quality, dim3(cdiv(a.n_seq, 64)), dim3(64), 0, s, a);
}

void launch_export_poses(const SeqState* state, float* xi_out, float* T_out, int n_seq, hipStream_t s, float* host_result, int host_tag)
{
    hipLaunchKernelGGL(k_export_poses, dim3(cdiv(n_seq, 64)), dim3(64), 0, s, state, xi_out, T_out, n_seq, host_result, host_tag);
}

void launch_se3(int op, const float* a, const float* b, float* out, hipStream_t s)
{
    hipLaunchKernelGGL(k_se3, dim3(1), dim3(64), 0, s, op, a, b, out);
}
void launch_pose_algebra(int op, int n, const double* in, double* out, hipStream_t s)
{
    hipLaunchKernelGGL(k_pose_algebra, dim3((n + 63) / 64), dim3(64), 0, s, op, n, in, out);
}

}  // namespace dvo
