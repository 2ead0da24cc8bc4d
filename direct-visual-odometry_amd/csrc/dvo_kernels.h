// dvo_kernels.h -- argument blocks and launch wrappers of the HIP kernels (dvo_kernels.hip).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/dvo.h"
#include "dvo_math.h"

namespace dvo {

// Per-sequence tracker state, resident on the device for the whole coarse-to-fine loop.
struct SeqState {
    float xi[6];   // current relative twist (tracker.cpp:28,48)
    Pose  pose;    // exp(-xi) rounded to float: what every warp of the level uses
    int   active;  // 0 once the level's stop test fired (tracker.cpp:68-73)
    int   iter;    // iterations done on the current level
    double Tc[12]; // exp(+xi) in double (R row major, then t): carried so each iteration evaluates 2 exps instead of 4
};

struct PyramidArgs {
    const float* src[3];               // gray, depth, sigma at input resolution [n_seq][src_h][src_w] (nullptr = skip)
    float* dst[3][DVO_MAX_LEVELS];     // per map, per level [n_seq][h][w]
    int src_w, src_h, culls, levels;
    int w[DVO_MAX_LEVELS], h[DVO_MAX_LEVELS];
    float inv_tw;                      // 1 / top-level width
    int n_seq = 0;                     // set by launch_pyramid
    // optional (wgt[0] != nullptr, depth and sigma present): also write the k_prep_ref map of every level
    float* wgt[DVO_MAX_LEVELS];
    float step[DVO_MAX_LEVELS];
    float sigma_min, sigma_max;
    // optional raw sensor input (raw_rgb != nullptr; src[] is then ignored): the conversion of k_ingest (loader.cpp:55-60,137-147,
    // transform.cpp:60-76) is applied to the 1/4^culls of the pixels the pyramid keeps, while they are loaded -- the float maps
    // of the full frame are never materialised.  raw_depth == nullptr: gray only (mono).
    const uint8_t* raw_rgb;      // [n_seq][src_h][src_w][raw_channels], channels 1 (gray), 3 (R,G,B) or 4 (R,G,B,A)
    const uint16_t* raw_depth;   // [n_seq][src_h][src_w]
    int raw_channels, raw_invalidate_gray;
    // the input buffers (raw or float) hold src_img_rows rows per image and top-level row y comes from stored row y << src_row_shift:
    // (src_h, culls) for a whole frame, (src_h >> culls, 0) when the host uploaded only the rows the pyramid keeps (upload_rows)
    int src_img_rows, src_row_shift;
    float raw_gray_scale, raw_depth_scale, raw_sigma_valid, raw_sigma_invalid;
    // optional copy-forward (Batch plan, seq_action != nullptr): the workgroups of a sequence whose effective action is DVO_SEQ_SKIP
    // read no input; they write what a build writes, taken from the reference set (same layout): gray / depth / sigma at the top
    // level (lower levels are pass_valid of it, which is what a build stores there) and wgt level by level.
    const uint8_t* seq_action;                 // [n_seq] effective action (k_plan)
    const float* ref[3][DVO_MAX_LEVELS];       // gray, depth, sigma of the reference set
    const float* ref_wgt[DVO_MAX_LEVELS];
    // optional lens undistortion (remap != nullptr; whole frames): k_pyramid_remap (mono frames: gray only; with a plan
    // k_pyramid_remap_plan) or, with depth (raw_depth or src[1] set), k_pyramid_remap_depth gathers each kept pixel through its
    // sequence's camera table (k_undistort_map) -- launch_pyramid then never picks k_pyramid / k_pyramid_raw4
    const int* remap = nullptr;       // [n_cam][th][tw] source index into the full frame, -1 = border (INVALID)
    const int* remap_cam = nullptr;   // [n_seq] camera (table) of each sequence
};

// Photometric calibration of raw mono frames (dvo_batch_set_photometric, dvo_vo_set_photometric): the second
// argument block of the k_pyramid*_photo kernels, beside PyramidArgs (which stays as it is for every other kernel).  Set (gain !=
// nullptr) only on a handle with a calibration: launch_pyramid then takes the photo kernels, and only them.
//   gray = response[seq_cal[s]][g8] * gain[seq_pair[s]][y][x]        (one multiply; gain < 0: the pixel is DVO_INVALID)
struct PhotoArgs {
    const float* response = nullptr;   // [n_cal][256] inverse response in gray units
    const float* gain = nullptr;       // [n_pair][th][tw] 1 / vignette at the kept pixel's source, kPhotoMasked where there is none
    const int* seq_cal = nullptr;      // [n_seq] calibration of each sequence
    const int* seq_pair = nullptr;     // [n_seq] gain table (calibration x undistortion camera) of each sequence
};
constexpr float kPhotoMasked = -1.0f;  // gain of a masked pixel (vignette not finite or <= 0) or of the remap's border: no 1 / V is negative

// One distinct camera of the fused undistortion: the full-resolution K (fx, fy, cx, cy) and D = (k1, k2, p1, p2, k3)
struct UndistortCam {
    Intr k;
    float D[5];
};

// Grids of the per-(sequence, pixel) kernels: x = workgroups of one sequence, (y, z) = the sequence -- seq = z * 32768 + y, so the
// sequence index costs no division and is not capped by the 65 535 limit of one grid dimension.  Kernels return for seq >= n_seq.
#define DVO_GRID_SEQ_Y 32768u
#ifdef __HIPCC__
inline dim3 seq_grid(unsigned blocks_per_seq, unsigned n_seq)
{
    const unsigned gy = n_seq < DVO_GRID_SEQ_Y ? (n_seq ? n_seq : 1u) : DVO_GRID_SEQ_Y;
    return dim3(blocks_per_seq ? blocks_per_seq : 1u, gy, (n_seq + gy - 1u) / gy);
}

// Entry `i` of a per-sequence table the kernel only reads, at an index that is uniform across the workgroup: through the constant
// address space, so the loads are scalar (s_load into SGPRs) even after the kernel's own stores and atomics, and with the index
// made provably uniform (readfirstlane of a value every lane holds) where it came from a list in memory.
template <class T>
__device__ __forceinline__ T load_seq_entry(const T* table, int i)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return ((const __attribute__((address_space(4))) T*)table)[__builtin_amdgcn_readfirstlane(i)];
#else
    return table[i];   // (the host pass only parses device code)
#endif
}
#endif

struct GnArgs {
    const float* obj_gray;   // level buffers [n_seq][h][w]
    const float* ref_gray;
    const float* ref_depth;
    const float* ref_wgt;    // step / clamp(ref_sigma)     (k_prep_ref); 1 / ref_depth is recomputed per pixel (recip_rn: the IEEE quotient)
    float wgt_const = 0.0f;  // ref_wgt == nullptr: the weight of every pixel that can contribute (FrameSet::sigma_by_validity)
    const SeqState* state;
    float* partials;         // [n_seq][nblk][32]
    uint8_t* mask;           // optional [n_seq][h][w], pre-zeroed
    int w, h, nblk;
    float inv_w;
    int q256, r256;          // 256 / w and 256 % w: a thread's next pixel is 256 further in raster order
    Intr k;
    GnParams prm;
    int ignore_active;       // 1 on the first iteration of a level / probes (k_track_gn_tile only; k_track_gn uses `list`)
    // k_track_gn is launched with a fixed, resident-sized grid whose workgroups stride over the tiles of the ACTIVE
    // sequences only.  list = nullptr: all n_seq sequences; else list[0] = count and list[4..] = sequence ids
    // (written by the previous k_gn_solve).  next_count, if set, is zeroed for the k_gn_solve that follows.
    const int* list = nullptr;
    int* next_count = nullptr;
    int n_seq = 1;
    // The level's tile geometry, filled by Tracker::gn_args from the GnTiling that Tracker::init stored (the solve that sums the rows
    // gets the same blk_first / blk_count from Tracker::solve_args).  k_track_gn_tile reads none of it.
    int blk_first = 0, blk_count = 0;  // live tiles of a sequence
    int t_shift = 6, x_org = 0, y_org = 0;  // 2-D tiles (with tiles_x below): see GnTiling
    // k_track_gn_tile: 64 x (4*PPT) pixel tiles with the reference patch staged in LDS, nblk = tiles_x * tiles_y (gn_tile_geometry);
    // the other kernels: tiles_x = GnTiling::tiles_x of a level with 2-D tiles, else 0
    int tiles_x, tiles_y;
    int margin;              // patch = tile grown by margin+1 (left/top) and margin+2 (right/bottom) pixels
    // Batch plan: the effective action of each sequence of the launch (k_plan); only DVO_SEQ_TRACK sequences start a level.  Read by the
    // kernels that test per-sequence flags (k_track_gn_tile, k_track_gn_fused, k_track_level); k_track_gn gets the plan's list instead.
    const uint8_t* plan_action = nullptr;
    // Per-sequence intrinsics (dvo_batch_set_intrinsics): the level's row of the Batch table, one Intr per sequence of the launch.
    // Set: the per-camera instantiations run and load seq_k[seq] once per workgroup (scalar loads); nullptr: every sequence uses `k`.
    const Intr* seq_k = nullptr;
};

struct PrepArgs {  // per-pixel constants of a reference frame, all levels in one launch
    const float* depth;      // level buffers are contiguous: [level][n_seq][h][w]
    const float* sigma;
    float* wgt;
    size_t level_end[DVO_MAX_LEVELS];  // cumulative element count after each level
    float step[DVO_MAX_LEVELS];
    float sigma_min, sigma_max;
    int levels;
};

struct SolveArgs {
    SeqState* state;
    const float* partials;
    dvo_track_log* log;        // optional [n_seq]
    dvo_gn_result* result;     // optional [n_seq]
    unsigned long long* counters;  // optional: [0] += level_pixels, [1] += 1 per solved sequence-iteration
    int nblk, level, level_pixels;
    int max_iterations, fixed_iterations;
    float min_update, min_residual;
    int ignore_active;         // 1 on the first iteration of a level: every sequence restarts (iter = 0)
    // active-sequence lists ([0] = count, [4..] = ids): workgroup b handles list_in[4 + b] (nullptr: sequence b) and
    // appends its sequence to list_out while it stays active (order is irrelevant to the results)
    const int* list_in = nullptr;
    int* list_out = nullptr;
    int* progress = nullptr;   // optional, mapped HOST memory: workgroup 0 stores (sequences this iteration evaluated + 1)
    int n_seq = 1;             // sequences of the launch (set by launch_gn_solve)
    int blk_first = 0, blk_count = -1;  // partial rows outside [blk_first, blk_first + blk_count) count as zero (-1: all rows)
    long long* dbg_stamp = nullptr;     // diagnostic (k_track_persist's timeline): [0] after the 6x6 solve, [1] after the pose update
};

// Robust residual weights (dvo_batch_set_robust_weights).  One entry per sequence: the constants of the weight
// rho(r) the sequence's next k_track_gn_rw launch applies.  kind = DVO_ROBUST_NONE: rho = 1 ("plain"), whatever the batch's kind.
struct RobustEntry {
    int kind;      // DVO_ROBUST_NONE / HUBER / STUDENT_T
    float A, B;    // Huber: A = c = k * sqrtf(s2); Student-t: A = (nu + 1) * s2, B = nu * s2
    float s2;      // the squared scale the constants came from; +inf for a plain entry
};
// The entry of (kind, param, s2).  A scale that is not finite and > 0 gives the plain entry.
DVO_HD RobustEntry robust_entry(int kind, float param, float s2)
{
    RobustEntry e;
    e.kind = DVO_ROBUST_NONE; e.A = 0.0f; e.B = 0.0f; e.s2 = __builtin_inff();
    if (kind == DVO_ROBUST_NONE || !(s2 > 0.0f) || !(s2 < __builtin_inff())) return e;
    e.kind = kind; e.s2 = s2;
    if (kind == DVO_ROBUST_HUBER) e.A = param * sqrtf(s2);
    else { e.A = (param + 1.0f) * s2; e.B = param * s2; }
    return e;
}
// rho(r) of one pixel: Huber fabsf(r) <= c ? 1 : c / fabsf(r); Student-t A / fmaf(r, r, B); plain 1.  One IEEE division serves both
// kinds (the entry is wave-uniform, so the selects around it are scalar).
DVO_HD float robust_rho(const RobustEntry& e, float r)
{
    const float ar = fabsf(r);
    const float den = e.kind == DVO_ROBUST_STUDENT_T ? fmaf(r, r, e.B) : ar;
    const float q = e.A / den;
    const bool one = (e.kind == DVO_ROBUST_NONE) | ((e.kind == DVO_ROBUST_HUBER) & (ar <= e.A));
    return one ? 1.0f : q;
}
struct RobustGn {      // second argument of k_track_gn_rw / k_track_gn_rw_cam
    const RobustEntry* table;   // [n_seq of the launch], indexed like GnArgs::state
};
struct RobustSolve {   // second argument of k_gn_solve_rw
    RobustEntry* table;         // indexed like SolveArgs::state
    float* last_s2;             // [n_seq]: the s2 each sequence's last evaluated iteration used (+inf: plain)
    int kind, adaptive;         // adaptive: the solve writes the next entry from this iteration's residual
    float param, floor2;
};
struct RobustBeginArgs {   // k_robust_begin: the table at the start of a tracking call
    RobustEntry* table; float* last_s2;
    const float* scales;   // GIVEN: [n_seq] s (device), or nullptr: every sequence s2_all
    float s2_all;
    int n_seq, kind, given;
    float param;
};
void launch_robust_begin(const RobustBeginArgs& a, hipStream_t s);

// The median (MAD) robust scale (dvo_batch_set_robust_median; the contract is in include/dvo.h).  Every contributing
// pixel's |r| is binned, 16 bins per octave over [2^-16, 1), and the solve selects the median bin of the sequence's 256 exact counts:
// the next launch's RobustEntry comes from the bin's midpoint.  Integer and float32 only, so the host replica has the same bits.
#define DVO_MEDIAN_BINS 256
#define DVO_MEDIAN_K0 1776   /* (127 - 16) << 4: the exponent-and-4-mantissa-bits word of 2^-16 */
DVO_HD int median_bin(float r)
{
    unsigned u;
    const float ar = fabsf(r);
    __builtin_memcpy(&u, &ar, sizeof u);
    const int k = (int)(u >> 19) - DVO_MEDIAN_K0;
    return k < 0 ? 0 : (k > DVO_MEDIAN_BINS - 1 ? DVO_MEDIAN_BINS - 1 : k);
}
// s2 of median bin m: med = the bin's midpoint, s = 1.4826f * med, s2 = max(s * s, floor2) (no contraction: two roundings)
DVO_HD float median_s2(int m, float floor2)
{
    const unsigned u = ((unsigned)(m + DVO_MEDIAN_K0) << 19) | (1u << 18);
    float med;
    __builtin_memcpy(&med, &u, sizeof med);
    const float s = 1.4826f * med;
    const float s2 = s * s;
    return s2 > floor2 ? s2 : floor2;
}
struct MedianGn {      // last argument of k_track_gn_md / k_track_gn_md_cam
    unsigned* hist;             // [n_seq of the launch][256] counts, indexed like GnArgs::state; zero before the launch
};
struct MedianSolve {   // last argument of k_gn_solve_md
    unsigned* hist;             // [n_seq][256], indexed like SolveArgs::state: read, then zeroed for the next tile launch
    unsigned* hist_last;        // [n_seq][256]: the counts of each sequence's last evaluated iteration (not written by the priming pair)
    int* log;                   // optional [n_seq][levels][log_its][3]: (bits of the s2 used, m, n) of every logged iteration
    int* prime_mn;              // [n_seq][2]: (m, n) of the priming pair
    int* step_mn;               // optional [n_seq][2] (dvo_op_gn_step_robust_median): (m, n) of this solve
    int levels, log_its;
    int prime;                  // the priming pair: the entry and prime_mn only -- no pose, log, iteration count, list or record
};
struct MedianBeginArgs {   // k_median_begin: zero rows and priming slots at the start of a tracking call
    unsigned* hist; unsigned* hist_last; int* prime_mn;
    int n_seq;
};
void launch_median_begin(const MedianBeginArgs& a, hipStream_t s);

// Affine brightness compensation (dvo_batch_set_affine_brightness): I2(warp(x)) ~ a * I1(x) + b per sequence.  One
// entry per sequence: the (a, b) the sequence's next k_track_gn_ab launch applies; (1, 0) is the plain residual bit for bit.
struct AffineEntry {
    float a, b;
};
// A given row: (1, 0) unless both values are finite and a > 0.
DVO_HD AffineEntry affine_entry(float a, float b)
{
    AffineEntry e;
    const float inf = __builtin_inff();
    const bool ok = (a > 0.0f) & (a < inf) & (b > -inf) & (b < inf);
    e.a = ok ? a : 1.0f; e.b = ok ? b : 0.0f;
    return e;
}
#define DVO_AFFINE_MOMENTS 5   /* M0 = sum rho, M1 = sum rho I1, M2 = sum rho I2, M11 = sum rho I1 I1, M12 = sum rho I1 I2 */
// The brightness moments of a launch have partial rows of their own, [n_seq][nblk][8] (slots 5..7 zero), indexed like GnArgs::partials
// and reduced in the order of the 29 sums: wave, the four waves through LDS in wave order, then the tiles in double in the solve.
struct AffineGn {      // last argument of k_track_gn_ab / k_track_gn_ab_cam
    const AffineEntry* table;   // [n_seq of the launch], indexed like GnArgs::state
    float* moments;
    int prime;                  // the priming pair: rho = 1 whatever the robust entry says
};
struct AffineSolve {   // last argument of k_gn_solve_ab
    AffineEntry* table;         // indexed like SolveArgs::state
    const float* moments;       // indexed like SolveArgs::partials
    float* last;                // [n_seq][2]: the entry each sequence's last evaluated iteration used ((0, 0): not tracked)
    float* log;                 // optional [n_seq][levels][log_its][2]: the entry every logged iteration used
    float* prime_ab;            // [n_seq][2]: the entry the priming pair wrote
    double* moments_out;        // optional [n_seq][5] (dvo_op_gn_step_affine); [0] = the N of the closed form
    int levels, log_its;
    int estimate;               // the solve writes the next entry from this iteration's moments (else the entry stays: GIVEN)
    int prime;                  // the priming pair: the entry and prime_ab only -- no pose, log, iteration count, list or record
    int robust;                 // robust weights are on too: N = M0 and the RobustEntry is kept as k_gn_solve_rw keeps it
    int min_pixels;
    float min_contrast, gain_min, gain_max;
};
struct AffineBeginArgs {   // k_affine_begin: the table at the start of a tracking call
    AffineEntry* table; float* last; float* prime_ab;
    const float* rows;     // GIVEN: [n_seq][2] (device), or nullptr: every sequence (a_all, b_all)
    float a_all, b_all;
    int n_seq;
};
void launch_affine_begin(const AffineBeginArgs& a, hipStream_t s);

// The geometric (depth) term of a sensor-depth batch (dvo_batch_set_geometric).  While on, GnArgs::ref_depth / ref_wgt /
// wgt_const hold the TRACKED frame's own maps and the reference's depth is sampled at the warped position: its base comes in this
// block, a further kernel argument (GnArgs keeps its layout).  The two new sums S29 = sum rg^2 and S30 = n_geo take slots 29 and 30
// of the 32-float partial row.
struct GeoGn {         // last argument of k_track_gn_z / k_track_gn_z_cam
    const float* ref_z;   // [n_seq of the launch][h][w] reference depth of the level, indexed like GnArgs::ref_gray
    float weight;         // >= 0
    float max_diff;       // > 0: |rz| above it has no geometric row
};
struct GeoSolve {      // last argument of k_gn_solve_z
    float* last;          // [n_seq][2]: (n_geo, S29) of each sequence's last evaluated iteration ((0, 0): not tracked), like SolveArgs::state
    float* log;           // optional [n_seq][levels][log_its][2]: (n_geo, S29) of every logged iteration
    double* sums_out;     // optional [n_seq][2] (dvo_op_gn_step_geometric): (n_geo, S29) in double
    int levels, log_its;
};

// Step control: damped Gauss-Newton with step acceptance (dvo_batch_set_step_control; the contract is in include/dvo.h).
// One dvo_lm_entry per sequence: the accepted pose, its sums and lambda.  The tile kernel is the plain k_track_gn; only the solve
// differs.  Float32 and integer decisions, so the host replica has the same bits.
struct LmSolve {       // last argument of k_gn_solve_lm
    dvo_lm_entry* table;        // indexed like SolveArgs::state
    dvo_lm_record* last;        // [n_seq]: decision counts, lambda and the finest level's accepted residual (n_first == 0: not tracked)
    int* log;                   // optional [n_seq][levels][log_its][2]: (bits of the lambda the solve used, decision) of every logged iteration
    float* upd_out;             // optional [n_seq][6] (dvo_op_lm_step): the step
    int* decision_out;          // optional [n_seq] (dvo_op_lm_step)
    int levels, log_its;
    float lambda_up, lambda_down, lambda_floor, lambda_max, min_valid_fraction;
};
struct LmBeginArgs {   // k_lm_begin: the table and the records at the start of a tracking call
    dvo_lm_entry* table; dvo_lm_record* last;
    float lambda0;
    int n_seq;
};
void launch_lm_begin(const LmBeginArgs& a, hipStream_t s);
// dvo_op_lm_step: k_gn_solve_lm's serial tail on given sums, one case per thread.  a.state: [n] scratch SeqState, set up by the kernel
// from xi_eval (Tc = exp(xi), pose = float(exp(-xi)), iter = it_prev); m.table: the entries, updated in place.
void launch_lm_step(const SolveArgs& a, const LmSolve& m, const double* sums, const float* xi_eval, int n, int it_prev, hipStream_t s);

// k_track_persist: the whole of Tracker::track for ONE sequence in one launch (a dvo_vo handle).
struct PersistLevel {
    const float* obj_gray; const float* ref_gray; const float* ref_depth; const float* ref_wgt;
    float wgt_const, inv_w;
    int w, h, nblk, q256, r256;
    Intr k;
    GnParams prm;
    int blk_first, blk_count, t_shift, x_org, y_org, tiles_x, t2d, level_pixels;
};
struct MonoSeq;
struct AgeEntry;
struct PersistMono {       // optional tail of k_track_persist for a mono dvo_vo handle: what k_mono_decide does, by the solver's thread, in the
    MonoSeq* meta;         // same launch -- the pose, the keyframe decision and the world pose reach the host with the tracker's tag
    float ref_xi[6];       // the reference keyframe (the host keeps FrameHistory): MonoRef's fields
    int ref_id, n_total;
    int frame_id, max_frames;
    float min_translation;
    int enabled;
    // ... and k_age_table's (the per-keyframe relative poses of Mapper::update) when the frame is not a keyframe, by the solver's workgroup:
    const float* hist_xi;  // [n_hist][6], device copy of FrameHistory's poses (current: the host refreshed it before the launch); nullptr: not here
    AgeEntry* ages;        // [n_hist]
    int n_hist;
    int* zero_word;        // the valid-update counter of the depth update that follows (cleared here)
};
struct PersistArgs {
    PersistLevel lv[DVO_MAX_LEVELS]{};
    int levels;
    SeqState* state;       // [1]
    float* partials;       // [max nblk][32]
    dvo_track_log* log;    // [1]
    int* ctl;              // device memory, 64-byte aligned: the control line [0] epoch [1] next level [2] status [4..15] pose, then one arrival slot per workgroup
    int max_iterations, fixed_iterations;
    float min_update, min_residual;
    float* xi_out; float* T_out;
    float* host_result;    // fine-grained mapped host memory: [0..5] xi, [6..21] T, [22] tag, [23] tag of a launch that gave up;
                           // with `mono`: [24..29] frame_xi, [30..45] T_world, [46] need (written before the tag)
    PersistMono mono{};
    int host_tag;          // unique per launch: also the base of this launch's epoch numbers
    int spin_limit;        // polls of the epoch word before a workgroup gives up (every wait in the kernel is bounded)
    int dbg_worker;        // which tile worker leaves the stamps (DVO_PERSIST_TIMELINE=<index>; 0 owns a corner tile of every level)
    long long* dbg;        // optional [2][64][8] wall-clock stamps (100 MHz) of the solver and of worker 0 per step (tools/persist_timeline.py)
};
bool track_persist_available(int ppt, int group);
int  track_persist_max_grid(int ppt, int group, int* out);   // workgroups that are co-resident on the current device
bool launch_track_persist(const PersistArgs& p, int ppt, int group, int grid, hipStream_t s);

// Tile geometry of k_track_gn: the single source of tile counts for host and device code.
//  * raster tiles: 256 * ppt consecutive pixels (any size; tiles outside the crop rows are not live);
//  * 2-D tiles (ppt = 4): TW = 2^shift columns x (64 / TW) * 16 rows, lane = (column, row-in-wave), wave w owns pixel rows
//    w*4 .. w*4+3 of the lane's row set.  Used when the width is a multiple of 64, 32 or 16 (64 x 16, 32 x 32, 16 x 64 tiles),
//    the level has no crop window and is at least two tiles tall: only tiles on the image border hold border pixels.
struct GnTiling {
    int t2d = 0, shift = 6, tiles_x = 1, x_org = 0, y_org = 0;
    int count = 1;                        // tiles (= partial rows) per sequence
    int live_first = 0, live_count = 0;   // tiles that are launched and summed
    long long live_pixels = 0;            // image pixels they cover (profile counter)
};
inline GnTiling gn_tiling(int w, int h, int ppt, int crop)
{
    GnTiling t;
    const int npix = w * h;
    // (Tried: 32 x 32 tiles laid over the crop window [20,140] x [20,100] of the crop level, so that no tile touches the image
    // border and nothing outside the window is evaluated.  No measurable change -- that level's launches are latency chains,
    // not work -- so the crop level keeps raster tiles; x_org / y_org / shift stay general for it.)
    if (ppt == 4 && !crop && w >= 16 && (w % 16) == 0) {
        // the widest power-of-two tile width (<= 64) that divides the level width; rows per tile = (64 / TW) * 16, and the
        // tile must not be taller than about half the image (else every tile touches the top and bottom border anyway)
        const int shift = (w % 64) == 0 ? 6 : ((w % 32) == 0 ? 5 : 4);
        const int rows = (64 >> shift) * 16;
        if (rows * 2 <= h) {
            t.t2d = 1; t.shift = shift; t.tiles_x = w >> shift;
            t.count = t.tiles_x * ((h + rows - 1) / rows);
            t.live_first = 0; t.live_count = t.count; t.live_pixels = npix;
            return t;
        }
    }
    const int T = 256 * ppt;
    t.count = (npix + T - 1) / T;
    t.live_first = 0; t.live_count = t.count; t.live_pixels = npix;
    if (crop) {
        int lo = t.count, hi = -1;
        for (int b = 0; b < t.count; b++) {
            const int row0 = (b * T) / w;
            int last = b * T + T - 1;
            if (last > npix - 1) last = npix - 1;
            if (last / w >= 20 && row0 <= 100) { if (b < lo) lo = b; if (b > hi) hi = b; }
        }
        if (hi < lo) { t.live_count = 0; t.live_pixels = 0; return t; }
        long long p1 = (long long)(hi + 1) * T;
        if (p1 > npix) p1 = npix;
        t.live_first = lo; t.live_count = hi - lo + 1; t.live_pixels = p1 - (long long)lo * T;
    }
    return t;
}

// ------------------------------------------------------------------------------------------------
// Mapping (src/map/mapper.cpp, src/map/implement.cpp) for n_seq sequences at once.  Every map is [n_seq][h][w] (top pyramid level);
// a launch covers all sequences and each sequence takes part or not according to its own Mapper::needNewFrame flag, which
// lives on the device (MonoSeq::need): no host round trip between tracking and mapping.
// ------------------------------------------------------------------------------------------------
struct MonoSeq {          // Mapper + FrameHistory state of one sequence (mapper.cpp:16-60, frame.hpp:146-188)
    float ref_xi[6];      // Frame::m_xi of the newest keyframe           } the first 32 bytes are what a single dvo_vo handle
    int   ref_id;         // its Frame::id                                } uploads before k_mono_decide (its FrameHistory
    int   n_total;        // keyframes created so far                     } lives on the host)
    float frame_xi[6];    // m_xi of the frame being processed = concatenate(ref_xi, rel_xi), frame.cpp:7-14
    float rel_xi[6];      // m_relative_xi = Tracker::track's result
    Pose  rel_pose;       // exp(+rel_xi): the warp of Mapper::propagate (mapper.cpp:66) and Mapper::update (mapper.cpp:94)
    float T_world[16];    // exp(frame_xi), system.hpp:73
    int   frame_id;
    int   need;           // Mapper::needNewFrame (mapper.cpp:45-60) of this frame
    int   valid_updates;  // "valid update: N pixel", mapper.cpp:136
    int   clamped;        // cumulative: pixels whose age pointed past the keyframe ring and were searched against the oldest retained
                          // keyframe instead (UpdateArgs::clamp_age; 0 for a history that holds every keyframe, as the reference's)
};

// What System::VisualOdometry::odometrize does between Tracker::track and Mapper::estimate (system.hpp:57-73, frame.cpp:7-14,
// mapper.cpp:45-60) for one sequence, in the double-precision pose algebra of dvo_math.h: rel_xi <- the tracker's twist, frame_xi <-
// concatenate(ref_xi, rel_xi), need <- needNewFrame, rel_pose <- exp(+rel_xi), T_world <- exp(frame_xi).  Shared by k_mono_decide and
// k_track_persist's mono tail: the same operations, the same bits.
__device__ __forceinline__ int mono_decide_one(MonoSeq& m, const float rel[6], int frame_id, float min_translation, int max_frames, float fx[6],
                                               float T[16])
{
    float ref[6];
    for (int i = 0; i < 6; i++) ref[i] = m.ref_xi[i];
    se3_concatenate_f(ref, rel, fx);
    const double tn2 = (double)rel[0] * rel[0] + (double)rel[1] * rel[1] + (double)rel[2] * rel[2];
    const int need = (sqrt(tn2) > (double)min_translation || (frame_id - m.ref_id >= max_frames)) ? 1 : 0;  // mapper.cpp:45-60
    se3_exp_f(fx, T);
    Pose rp;
    pose_from_xi(rel, 1.0f, rp);
    for (int i = 0; i < 6; i++) { m.rel_xi[i] = rel[i]; m.frame_xi[i] = fx[i]; }
    m.rel_pose = rp;
    for (int i = 0; i < 16; i++) m.T_world[i] = T[i];
    m.frame_id = frame_id;
    m.need = need;
    m.valid_updates = 0;
    return need;
}

// The building blocks of the per-sequence bookkeeping kernels (k_mono_decide / k_mono_commit, their _plan forms and k_kf_decide), one
// thread per sequence s.  xi_world [n_seq][6], T_world [n_seq][16] and is_key [n_seq] are the call's outputs; one a caller does not
// want is null.
__device__ __forceinline__ void mono_identity_world(int s, float* xi_world, float* T_world)
{
    if (xi_world) for (int i = 0; i < 6; i++) xi_world[s * 6 + i] = 0.0f;
    if (T_world) for (int i = 0; i < 16; i++) T_world[s * 16 + i] = (i % 5 == 0) ? 1.0f : 0.0f;
}

// Start: the frame is frame `frame_id` and the first keyframe of the sequence, at the identity; `ring` = the sequence's [R][6] keyframe
// twists (slot 0 is written) or null.  MonoSeq::clamped is the caller's: a restart clears it, the first frame of a batch finds it 0.
__device__ __forceinline__ void mono_start_one(MonoSeq& m, int frame_id, float* ring, int s, float* xi_world, float* T_world, int* is_key)
{
    for (int i = 0; i < 6; i++) { m.ref_xi[i] = 0.0f; m.frame_xi[i] = 0.0f; m.rel_xi[i] = 0.0f; }
    for (int i = 0; i < 9; i++) m.rel_pose.R[i] = (i % 4 == 0) ? 1.0f : 0.0f;
    for (int i = 0; i < 3; i++) m.rel_pose.t[i] = 0.0f;
    for (int i = 0; i < 16; i++) m.T_world[i] = (i % 5 == 0) ? 1.0f : 0.0f;
    m.ref_id = frame_id; m.frame_id = frame_id; m.n_total = 1; m.need = 1; m.valid_updates = 0;
    if (ring) for (int i = 0; i < 6; i++) ring[i] = 0.0f;
    mono_identity_world(s, xi_world, T_world);
    if (is_key) is_key[s] = 1;
}

// Track: mono_decide_one on the tracker's twist, the frame's world pose and keyframe flag published.  Returns the flag.
__device__ __forceinline__ int mono_track_one(MonoSeq& m, const SeqState& st, int frame_id, float min_translation, int max_frames, int s,
                                              float* xi_world, float* T_world, int* is_key)
{
    float rel[6], fx[6], T[16];
    for (int i = 0; i < 6; i++) rel[i] = st.xi[i];
    const int need = mono_decide_one(m, rel, frame_id, min_translation, max_frames, fx, T);
    if (xi_world) for (int i = 0; i < 6; i++) xi_world[s * 6 + i] = fx[i];
    if (T_world) for (int i = 0; i < 16; i++) T_world[s * 16 + i] = T[i];
    if (is_key) is_key[s] = need;
    return need;
}

// FrameHistory::setRefFrame / push (frame.hpp:151-157): the frame becomes the reference keyframe and, with a ring (as mono_start_one's),
// its twist enters slot n_total % R.
__device__ __forceinline__ void mono_frame_to_ref(MonoSeq& m, float* ring, int R)
{
    const int slot = ring ? m.n_total % R : 0;
    for (int i = 0; i < 6; i++) {
        m.ref_xi[i] = m.frame_xi[i];
        if (ring) ring[slot * 6 + i] = m.frame_xi[i];
    }
    m.ref_id = m.frame_id;
    m.n_total += 1;
}

struct AgeEntry {      // one keyframe as seen from the current frame (Mapper::update, mapper.cpp:99-107)
    Pose  pose;        // exp(-r_xi), r_xi = concatenate(obj.xi, -born.xi)
    float tneg[3];     // -r_xi[0:3] (twist part; implement.cpp:56)
    int   slot;        // where the born keyframe's top-level gray lives: ring slot (batch) or history index (single handle)
};

// One entry of the age table (Mapper::update, mapper.cpp:99-107, hoisted out of the pixel loop): r_xi = concatenate(obj.xi, -born.xi), the
// pose exp(-r_xi) the epipolar search warps with and -r_xi's translation (implement.cpp:56).  Shared by k_age_table and k_track_persist's tail.
__device__ __forceinline__ void age_entry_one(const float frame_xi[6], const float* born_xi, int slot, AgeEntry& e)
{
    float ox[6], nb[6], r_xi[6];
    for (int k = 0; k < 6; k++) { ox[k] = frame_xi[k]; nb[k] = -born_xi[k]; }
    se3_concatenate_f(ox, nb, r_xi);
    pose_from_xi(r_xi, -1.0f, e.pose);
    for (int k = 0; k < 3; k++) e.tneg[k] = -r_xi[k];
    e.slot = slot;
}

struct AgeTableArgs {  // k_age_table: AgeEntry of every retained keyframe, once per frame and sequence (never per pixel)
    const MonoSeq* meta;
    const float* hist_xi;    // [n_seq][R][6], indexed by slot
    AgeEntry* ages;          // [n_seq][R], indexed by HISTORY index (0 = oldest retained keyframe)
    int n_seq, R;
    int n_hist;              // >= 0: explicit history length and slot = index (single handle); < 0: ring, length min(n_total, R)
    int* zero_word = nullptr; // optional: cleared by this launch (the single handle's valid-update counter, UpdateArgs::valid_updates)
};

// The culled top-level K of one sequence of a per-camera mono batch, as the mapping kernels read it (UpdateArgs::seq_K9)
struct MapK {
    float K9[9];
    int k_sparse;   // k9_sparse(K9)
};
// K9 = [fx 0 cx; 0 fy cy; 0 0 1] exactly: depthEstimate may skip the products with the zeros (UpdateArgs::k_sparse)
inline int k9_sparse(const float K9[9])
{
    return (K9[1] == 0.0f && K9[3] == 0.0f && K9[6] == 0.0f && K9[7] == 0.0f && K9[8] == 1.0f) ? 1 : 0;
}

struct UpdateArgs {
    float* ref_depth; float* ref_sigma; float* ref_age;   // [n_seq][h][w], in place (top level of the reference keyframes)
    const float* obj_gray;                                 // [n_seq][h][w]
    const AgeEntry* ages;            // [n_seq][R], index = history index (oldest first)
    const float* ring_gray;          // [n_seq][R][h][w]: top-level gray of the retained keyframes (batch), or nullptr
    const float* const* gray_table;  // [n_hist] device pointers (single handle / operator level), used when ring_gray == nullptr
    const MonoSeq* meta;             // rel_pose, rel_xi[2], n_total, need, valid_updates per sequence; nullptr: the explicit fields
    int n_seq, R, n_hist, w, h, crop, obj_id;
    int clamp_age;           // bounded history: a pixel born in a dropped keyframe searches the oldest retained one
    float inv_ww = 0.0f;     // 1 / width of the launched window (set by launch_depth_update)
    uint32_t seed;
    Intr k;
    float K9[9];
    int k_sparse = 0;        // K9 = [fx 0 cx; 0 fy cy; 0 0 1] exactly (set by launch_depth_update): depthEstimate skips the products with the zeros
    Pose rel_pose;           // exp(+rel_xi)          } operator level only (meta == nullptr)
    float rel_tz;            // rel_xi[2]             }
    int* valid_updates;      //                       }
    // Per-sequence intrinsics (dvo_batch_create_mono_cameras): the top-level row of the tracker's [level][n_seq] Intr table and
    // each sequence's culled top-level K9 + k_sparse.  Set: k_depth_update_cam runs and reads them instead of k / K9 / k_sparse.
    const Intr* seq_k = nullptr;
    const MapK* seq_K9 = nullptr;
};

struct PropArgs {      // Implement::propagate (implement.cpp:217-256)
    const float* ref_depth; const float* ref_sigma; const float* ref_age;   // [n_seq][h][w]
    float* depth; float* sigma; float* age;                                  // [n_seq][h][w]
    int* owner;                                                              // [n_seq][h][w] scratch
    int w, h, n_seq;
    Intr k;
    const MonoSeq* meta;     // per-sequence pose + need flag; nullptr: `pose` / `tz` below, unconditional
    Pose pose; float tz;
    float inv_w = 0.0f;      // 1 / w (set by launch_propagate_batch)
    // Compact list of the sequences that take this branch ([0] = count, [4..] = ids, written by k_mono_decide): the grid then holds
    // min(n_seq, n_slots) sequence slots and slot j works through list entries j, j + n_slots, ... -- on a typical frame a sixth of
    // the sequences create a keyframe, and a workgroup that only finds out it has nothing to do costs as much to dispatch as one
    // that works.  nullptr: every sequence (or its `meta` flag).
    const int* need_list = nullptr;
    int n_slots = 0;
    // Per-sequence intrinsics (dvo_batch_create_mono_cameras): [n_seq] top-level Intr.  Set: k_propagate_owner_cam warps with the
    // sequence's entry instead of `k`.
    const Intr* seq_k = nullptr;
};

#define DVO_PROMOTE_MAX_SEG 8
struct PromoteArgs {   // a tracked frame becomes the newest keyframe of the sequences whose need flag is set (mapper.cpp:23-27)
    const float* src[DVO_PROMOTE_MAX_SEG];   // [n_seq][count] blocks of the frame set ...
    float* dst[DVO_PROMOTE_MAX_SEG];         // ... copied over the same blocks of the reference set
    int count[DVO_PROMOTE_MAX_SEG];
    int n_seg, n_seq;
    const float* gray_top;   // [n_seq][npix] also pushed into the keyframe ring:
    float* ring_gray;        // [n_seq][R][npix], slot n_total % R
    int npix, R;
    const MonoSeq* meta;
    int all;                 // 1: every sequence (first frame), 0: need flag
    const int* need_list = nullptr;   // as PropArgs::need_list (all == 0 only)
    int n_slots = 0;
};

struct MonoRef { float ref_xi[6]; int ref_id, n_total, valid; };   // reference keyframe of a single dvo_vo handle (kernel argument)
void launch_mono_decide(MonoSeq* meta, const SeqState* state, int n_seq, int frame_id, float min_translation, int max_frames,
                        float* xi_world, float* T_world, int* is_key, const MonoRef* host_ref, hipStream_t s, int* need_list = nullptr);
void launch_mono_commit(MonoSeq* meta, float* hist_xi, int n_seq, int R, int all, int frame_id, float* xi_world, float* T_world, int* is_key,
                        hipStream_t s);
void launch_age_table(const AgeTableArgs& a, hipStream_t s);
void launch_promote(const PromoteArgs& a, hipStream_t s);
void launch_broadcast(const float* src, float* dst, int count, int n_seq, hipStream_t s);  // dst[seq][i] = src[i]
void launch_propagate_batch(const PropArgs& a, hipStream_t s);
void launch_regularize_batch(const float* depth, const float* sigma, int w, int h, int n_seq, float* out, hipStream_t s);
// Mapper::regularize + Frame::updateDepth / updateDepthSigma (mapper.cpp:139-144, frame.cpp:39-61) in one pass over the top level:
// the regularized depth goes to `depth_top_out` (a second top-level buffer: the stencil reads the old one) and, with the current
// sigma, to every lower level together with 1/depth and the weight.
struct RegDecArgs {
    const float* depth; const float* sigma;   // top level [n_seq][h][w], read only
    float* depth_top_out;                     // [n_seq][h][w]
    float* depth_lv[DVO_MAX_LEVELS]; float* sigma_lv[DVO_MAX_LEVELS]; float* wgt[DVO_MAX_LEVELS];  // per level (top: wgt only)
    int w[DVO_MAX_LEVELS], h[DVO_MAX_LEVELS], levels, n_seq;
    float step[DVO_MAX_LEVELS], sigma_min, sigma_max;
    float inv_w = 0.0f;                       // 1 / top-level width (set by the launch wrapper)
};
void launch_regularize_redecimate(const RegDecArgs& a, hipStream_t s);

// ---- the per-sequence plan of a mono batch (dvo_batch_set_mono_actions) ----------------------------------------------------------
// k_plan resolves the actions (has_ref = "has a keyframe"); these kernels replace k_mono_decide, k_mono_commit and
// k_regularize_redecimate in a planned call.  Plan state lives in separate per-sequence arrays, never in MonoSeq.
struct MonoPlanArgs {   // k_mono_decide_plan, k_mono_commit_plan
    MonoSeq* meta;
    const SeqState* state;
    const uint8_t* eff;      // [n_seq] effective action (k_plan)
    uint8_t* started;        // [n_seq] the sequence has started (read by decide, set by commit)
    int* need_save;          // [n_seq] MonoSeq::need of a sequence that does not track, restored by commit
    float* hist_xi;          // [n_seq][R][6]
    float* xi_world; float* T_world; int* is_key;
    int* need_list;          // as k_mono_decide's
    int n_seq, R, max_frames;
    float min_translation;
};
void launch_mono_decide_plan(const MonoPlanArgs& a, hipStream_t s);
void launch_mono_commit_plan(const MonoPlanArgs& a, hipStream_t s);
// k_kf_decide: both of them for a sensor-depth batch with keyframe tracking (dvo_batch_set_keyframe_tracking): meta, state, eff,
// xi_world, T_world, is_key, need_list (TRACK sequences whose rule fired, and the starts), n_seq, max_frames, min_translation
// (started, need_save, hist_xi and R are not used: a sequence has started once MonoSeq::n_total > 0)
void launch_kf_decide(const MonoPlanArgs& a, hipStream_t s);

// ---- keyframe depth fusion and keyframe carry of a sensor-depth batch ----------------------------------
// Both have a prep kernel (one thread per sequence, after k_kf_decide) that turns what k_kf_decide left -- eff, is_key, MonoSeq::rel_xi /
// rel_pose -- into one table entry per sequence, in a table of its own, and zeroes the sequence's record; the pixel kernels read the
// entry with a scalar load.
#define DVO_KF_FUSE_NONE  0   /* SKIP / BAD_ACTION, or a non-finite twist: nothing of the sequence is read or written */
#define DVO_KF_FUSE_CLEAR 1   /* a start or a promotion: the count plane becomes 0 */
#define DVO_KF_FUSE_FUSE  2   /* TRACK, rule not fired, finite twist */
#define DVO_KF_CARRY_NONE  0
#define DVO_KF_CARRY_CARRY 1  /* TRACK, rule fired, finite twist */
struct KfSeq {
    Pose F;     // float(exp(+xi)): MonoSeq::rel_pose, the T_rel of the push: keyframe -> tracked frame
    Pose Bk;    // float(exp(-xi)): pose_from_xi(xi, -1), what the tracker's kernels transform with: tracked frame -> keyframe
    int mode;   // DVO_KF_FUSE_* in the fusion's table, DVO_KF_CARRY_* in the carry's
    int pad[3];
};
struct KfRecord { int n_candidates, n_done, n_gated, pad; };   // n_done: dvo_kf_fusion_record::n_fused, dvo_kf_carry_record::n_carried
struct KfPrepArgs {
    const MonoSeq* meta;
    const uint8_t* eff;      // [n_seq] effective action of the push (k_plan)
    const int* is_key;       // [n_seq] k_kf_decide's keyframe flag
    KfSeq* table;            // [n_seq]
    KfRecord* rec;           // [n_seq]
    int n_seq;
};
// k_kf_fuse (dvo_batch_set_keyframe_fusion) clears, fuses or leaves.
struct KfFuseArgs {
    float* kf_depth[DVO_MAX_LEVELS];   // the keyframe set's depth pyramid, [n_seq][h_l][w_l], updated in place
    const float* frame_depth;          // the tracked set's top-level depth [n_seq][h][w] (never the keyframe set when a sequence fuses)
    uint8_t* counts;                   // [n_seq][h][w]
    const KfSeq* table;
    KfRecord* rec;
    const Intr* seq_k = nullptr;       // per-sequence top-level intrinsics [n_seq] (k_kf_fuse_cam), else k
    Intr k;
    int w[DVO_MAX_LEVELS], h[DVO_MAX_LEVELS], levels, n_seq;
    float inv_w = 0.0f;                // 1 / top-level width (set by launch_kf_fuse)
    float min_depth, max_diff;
    int max_count;
};
void launch_kf_fuse_prep(const KfPrepArgs& a, hipStream_t s);
void launch_kf_fuse(const KfFuseArgs& a, hipStream_t s);
// k_kf_carry (dvo_batch_set_keyframe_carry; before k_promote) blends the old keyframe's depth, warped into the tracked frame, into the
// tracked set's depth pyramid in place and stages the new counts; k_kf_carry_commit (after k_kf_fuse has cleared) copies the staged
// counts of the carrying sequences over the count plane.
struct KfCarryArgs {
    float* frame_depth[DVO_MAX_LEVELS];   // the tracked set's depth pyramid, [n_seq][h_l][w_l], updated in place
    const float* kf_depth;                // the old keyframe's top-level depth [n_seq][h][w] (never the tracked set when a sequence carries)
    const uint8_t* counts;                // the old keyframe's counts [n_seq][h][w]
    uint8_t* staged;                      // the new counts [n_seq][h][w]
    const KfSeq* table;
    KfRecord* rec;
    const Intr* seq_k = nullptr;          // per-sequence top-level intrinsics [n_seq] (k_kf_carry_cam), else k
    Intr k;
    int w[DVO_MAX_LEVELS], h[DVO_MAX_LEVELS], levels, n_seq;
    float inv_w = 0.0f;                   // 1 / top-level width (set by launch_kf_carry)
    float min_depth, max_diff;
    int max_count;
};
struct KfCarryCommitArgs {
    const uint8_t* staged;
    uint8_t* counts;
    const KfSeq* table;
    int npix, n_seq;
};
void launch_kf_carry_prep(const KfPrepArgs& a, hipStream_t s);
void launch_kf_carry(const KfCarryArgs& a, hipStream_t s);
void launch_kf_carry_commit(const KfCarryCommitArgs& a, hipStream_t s);
// ---- keyframe maps as compacted world-frame point clouds (dvo_batch_export_points) ---------------------------------
// k_points_prep (one thread per sequence) selects the sequence, writes Wk = float(exp(-ref_xi)) to its table entry and zeroes its
// total.  k_points_count (grid = chunks x sequences, a chunk = 256 lanes x 4 consecutive pixels of the linearly addressed level
// plane) evaluates the gates and writes one count per chunk; the counts of a sequence are also added to its total (an integer sum:
// order-free).  k_points_scan (one workgroup) turns the totals into offsets [n_seq + 1].  k_points_write evaluates the gates again,
// sums its sequence's chunk counts below its own in its head, ranks its points, stages them in LDS in rank order and stores them with
// consecutive lanes on consecutive points.  Nothing is ordered by an atomic.
#define DVO_POINTS_PER_THREAD 4
#define DVO_POINTS_CHUNK (256 * DVO_POINTS_PER_THREAD)
#define DVO_POINTS_MAX_PLANE (1 << 24)   /* split_row's range: pixels of one level plane */
inline int points_chunks(int w, int h) { return (w * h + DVO_POINTS_CHUNK - 1) / DVO_POINTS_CHUNK; }
struct PointsSeq {
    Pose Wk;    // float(exp(-ref_xi)): pose_from_xi(ref_xi, -1), keyframe camera -> world
    int on;     // the sequence contributes: started, and under DVO_POINTS_NEW its keyframe flag is set
    int pad[3];
};
struct PointsPrepArgs {
    const MonoSeq* meta;
    const uint8_t* started;   // [n_seq] (a planned mono batch); nullptr: started_by_total, else every sequence
    int started_by_total;     // a sequence has started once MonoSeq::n_total > 0 (sensor depth, as k_kf_decide)
    const int* is_key;        // [n_seq] keyframe flag of the last push / call
    int select_new;           // DVO_POINTS_NEW
    PointsSeq* table;         // [n_seq]
    uint32_t* seq_total;      // [n_seq] zeroed here
    int n_seq;
};
struct PointsArgs {
    const float* depth; const float* gray;   // the level's planes [n_seq][h][w]
    const float* sigma;                      // mono: the level's sigma plane (gate and / or output), else nullptr
    const float* age;                        // the age gate's plane (min_age > 0), else nullptr
    const uint8_t* counts;                   // the count gate's plane (min_count > 0), else nullptr
    const PointsSeq* table;
    uint32_t* chunk_count;                   // [n_seq][chunks]
    uint32_t* seq_total;                     // [n_seq]
    uint32_t* offsets;                       // [n_seq + 1] (the handle's)
    float* xyzg; uint32_t* src; float* sigma_out;   // [capacity][4], [capacity] or nullptr, [capacity] or nullptr
    uint32_t capacity;
    const Intr* seq_k = nullptr;             // per-sequence intrinsics of the level [n_seq] (k_points_write_cam), else k
    Intr k;
    int w, h, n_seq, stride, min_count, gate_sigma;
    int chunks = 0;                          // points_chunks(w, h)   } set by launch_points
    float inv_w = 0.0f;                      // 1 / w                 }
    float min_depth, max_depth, max_sigma, min_age;
};
void launch_points_prep(const PointsPrepArgs& a, hipStream_t s);
// count, scan and (capacity > 0) write; offsets_out: the caller's copy of the offsets [n_seq + 1]
void launch_points(const PointsArgs& a, uint32_t* offsets_out, hipStream_t s);
// k_regularize_redecimate_plan: k_regularize_redecimate for the TRACK sequences; a SKIP sequence copies its top-level depth forward to
// depth_top_out (nothing else is written); a RESTART sequence starts: its keyframe becomes the frame's gray pyramid (ring slot 0 too),
// the start map's depth and sigma with every level re-decimated and the weights, age 0 (the first frame of system.hpp:49-54).
struct MonoStartArgs {
    const uint8_t* eff;            // [n_seq] effective action (k_plan)
    const uint8_t* started;        // [n_seq] the sequence started before this call (its first start keeps its own top-level maps)
    const float* start_depth;      // optional [n_seq][h][w] (dvo_batch_set_mono_start_depth_device), with start_sigma
    const float* start_sigma;
    const float* init_depth;       // [h][w] the start map of a later start: the host map of dvo_batch_set_initial_depth, else the default
    const float* init_sigma;
    float* sigma_top;              // the keyframes' top-level sigma (= RegDecArgs::sigma, written for the starts only)
    float* age;                    // the keyframes' age map [n_seq][h][w]
    const float* frm_gray[DVO_MAX_LEVELS];
    float* ref_gray[DVO_MAX_LEVELS];
    float* ring_gray;              // [n_seq][R][h][w]
    int R;
};
void launch_regularize_redecimate_plan(const RegDecArgs& a, const MonoStartArgs& p, hipStream_t s);

// Which kernel a build ran: kind = DVO_PYRAMID_KERNEL_* (include/dvo.h), culls = the CULLS instance of the raw4 family (0: the kernel has
// none), plan = the PLAN instance.  Said by the launcher that made the choice, where it made it (dvo_op_pyramid_frames reports it).
struct PyramidKernel {
    int kind = DVO_PYRAMID_KERNEL_SCALAR, culls = 0, plan = 0;
};
// The pyramid-build family: nine kernel templates, 24 instances, over one set of device helpers (raw_luma8,
// raw_convert, RawWords, walk_levels, seq_skips) and one set of launcher helpers (pyramid_raw4_possible, aligned16, pyramid_grid,
// with_flag, with_culls).  launch_pyramid picks: with a remap k_pyramid_remap_depth<4 or 1, plan> (depth present) or
// k_pyramid_remap / k_pyramid_remap_plan (mono); else k_pyramid_raw4<culls, plan> where the four-pixel build is possible
// (pyramid_raw4_possible: 1-channel bytes, culls 1 or 2, whole groups of four kept pixels, 16-byte aligned input and tops), else
// k_pyramid<plan>.
// photo (optional, photo->gain set): raw mono frames of a calibrated handle -- k_pyramid_raw4_photo<2, plan> (kind _PHOTO_RAW4) where
// the four-pixel build is possible at culls 2 and the gain rows can be read 16 bytes at a time, else k_pyramid_photo<plan, remap>
// (_PHOTO_SCALAR, or _PHOTO_REMAP with a.remap).  Without it: exactly the kernels chosen before there was a calibration.
// filter (DVO_PYRAMID_FILTER_*; not NONE only without a remap and without a photo block): the binomial-filtered gray pyramid of
// DESIGN.md §39 -- k_pyramid_filter_top<culls, raw, plan, wide> and one k_pyramid_filter_down<plan> per lower level (kind _FILTER,
// plan = PLAN | WIDE << 1 | RAW << 2).  NONE: exactly the launches above.
PyramidKernel launch_pyramid(const PyramidArgs& a, int n_seq, hipStream_t s, const PhotoArgs* photo = nullptr,
                             int filter = DVO_PYRAMID_FILTER_NONE);
// k_photometric_map: gain[p][y][x] of pair p = (cal, cam) = 1 / vignette[cal][source of kept pixel (x, y)], the source being
// (x, y) << culls, or remap[cam][y][x] with a remap (then -1 gives kPhotoMasked).  vignette == nullptr: 1.
void launch_photometric_map(const float* vignette, const int* pairs /*[n_pair][2]*/, int n_pair, int w, int h, int culls, int tw, int th,
                            const int* remap, float* gain, hipStream_t s);
// The split build: launch_pyramid_coarse (k_pyramid_raw4_coarse: the gray maps below the top level) and
// launch_pyramid_rest (k_pyramid_raw4_rest: everything else) together write what launch_pyramid writes.  pyramid_can_split: the
// arguments are those of a plain raw build with depth (no plan, no remap) for which the four-pixel build is possible
// (pyramid_raw4_possible: stage B), and stage A's own conditions hold: eight top-level pixels per thread, level top - 1 exactly half
// as wide, its map 16-byte aligned.
bool pyramid_can_split(const PyramidArgs& a);
void launch_pyramid_coarse(const PyramidArgs& a, int n_seq, hipStream_t s);
void launch_pyramid_rest(const PyramidArgs& a, int n_seq, hipStream_t s);

// k_plan: the per-sequence actions of one Batch push (dvo_batch_set_actions), resolved on the device before the pyramid is built.
struct PlanArgs {
    const uint8_t* actions;  // [n_seq] requested actions; nullptr = every sequence DVO_SEQ_TRACK
    uint8_t* has_ref;        // [n_seq] in / out: the sequence has a reference frame
    uint8_t* eff;            // [n_seq] out: effective action (DVO_SEQ_SKIP / TRACK / RESTART)
    int* status;             // [n_seq] out: DVO_SEQ_TRACKED / SKIPPED / STARTED / BAD_ACTION
    SeqState* state;         // [n_seq] what k_track_begin writes; active = 1 for tracked sequences only
    dvo_track_log* log;      // [n_seq] levels + n_iter reset
    int levels;
    int* lists;              // n_sub lists of list_stride ints ([0] = count, [4..] = local ids): the tracked sequences per sub-batch
    int* lists_clear;        // the other set of lists: their counts are cleared here for the next plan
    int list_stride, n_sub, n_seq;
    int* tally;              // optional (with `ready`): two device counters, zero between launches
    int* ready;              // optional, mapped HOST memory: the last workgroup stores (tracked sequences + 1)
    const uint8_t* cam_changed;  // optional [n_seq]: 1 = the sequence's intrinsics change at this push, so it loses its reference first
};
void launch_plan(const PlanArgs& a, hipStream_t s);

// k_seed_pose (sensor depth) / k_mono_seed (mono): the start pose of one push (dvo_batch_set_pose_guess_mode), one
// thread per sequence, launched after k_track_begin / k_plan.  Each first folds the previous push into the sequence's history (from
// that push's effective action and result), then loads the start of every TRACK sequence into its SeqState as k_set_pose does.  A zero
// start writes nothing: the state stays exactly what k_track_begin / k_plan left.  History lives here, never in SeqState or MonoSeq.
struct PoseSeedArgs {
    SeqState* state = nullptr;       // [n_seq]
    const uint8_t* eff = nullptr;    // [n_seq] effective action of this push (k_plan); nullptr: every sequence takes `all_eff`
    int all_eff = DVO_SEQ_TRACK;
    int mode = 0;                    // DVO_GUESS_*
    const float* rows = nullptr;     // DVO_GUESS_GIVEN: [n_seq][6] the rows of this push; nullptr: none (zero start)
    float* start = nullptr;          // [n_seq][6] out: the start of each TRACK sequence, zero for the others
    uint8_t* prev_eff = nullptr;     // [n_seq] in: the previous push's effective action (0xff: none to fold in); out: this push's
    const float* last_xi = nullptr;  // [n_seq][6] what the previous push returned: relative twists (Tracker::xi_out) / world twists
    float* hist = nullptr;           // [n_seq][12] sensor depth: [0..5] the last tracked relative twist; mono: w1, then w2
    uint8_t* hist_n = nullptr;       // mono: [n_seq] world twists held in hist (0, 1, 2)
    const MonoSeq* meta = nullptr;   // mono: the keyframe twist ref_xi of each sequence
    int n_seq = 0;
};
void launch_seed_pose(const PoseSeedArgs& a, hipStream_t s);
void launch_mono_seed(const PoseSeedArgs& a, hipStream_t s);

// k_track_quality: the dvo_track_quality records of a batch's last push (dvo_batch_set_track_quality), one thread per
// sequence, launched by a read.  Reads the finest level's last solve (SolveArgs::result, kept by Tracker::quality), the track log and
// the push's status; writes the records straight into `out` (the caller's device buffer, or the staging of a host read).
struct QualityArgs {
    const dvo_gn_result* rec = nullptr;   // [n_seq] the sums of each sequence's last finest-level solve
    const dvo_track_log* log = nullptr;   // [n_seq]
    const int* status = nullptr;          // [n_seq] DVO_SEQ_TRACKED ... of the push; nullptr: every sequence has `all_status`
    int all_status = DVO_SEQ_TRACKED;
    dvo_track_quality* out = nullptr;     // [n_seq]
    int levels = 0;                       // the finest level is levels - 1
    int max_iterations = 0, fixed_iterations = 0;
    float min_update = 0.0f, min_residual = 0.0f;
    int n_seq = 0;
};
void launch_track_quality(const QualityArgs& a, hipStream_t s);
#ifdef __HIPCC__
// the state k_set_pose loads for twist x (not `active` / `iter`: k_track_begin / k_plan set them), and x as the reported start; a zero
// twist writes neither the state nor anything but +0 to `start`
__device__ __forceinline__ void seed_state(SeqState& st, float x[6], float* start)
{
    bool finite = true, zero = true;
    for (int i = 0; i < 6; i++) { finite = finite && isfinite(x[i]); zero = zero && x[i] == 0.0f; }
    if (!finite || zero) {
        for (int i = 0; i < 6; i++) start[i] = 0.0f;
        return;
    }
    double xd[6], R[9], t[3];
    for (int i = 0; i < 6; i++) { start[i] = x[i]; st.xi[i] = x[i]; xd[i] = x[i]; }
    pose_from_xi(x, -1.0f, st.pose);
    se3_exp_d(xd, R, t);
    for (int i = 0; i < 9; i++) st.Tc[i] = R[i];
    for (int i = 0; i < 3; i++) st.Tc[9 + i] = t[i];
}
#endif
void launch_cull(const float* src, int w, int h, int times, float* dst, hipStream_t s);
void launch_gradient(const float* img, int w, int h, int xdir, float* out, hipStream_t s);
void launch_warp_image(const float* gray, const float* depth, int w, int h, const Intr& k, const Pose& pose, float* out, hipStream_t s);
int  gn_blocks_per_seq(int w, int h, int ppt, int crop);  // = gn_tiling(...).count
// The launchers below take GnArgs / SolveArgs complete (Tracker::gn_args, Tracker::solve_args) and set only what is theirs: n_seq, the
// grid, and the fields their schedule does not use (list, next_count, mask, list_in / list_out, progress).  ppt, group and t2d (the
// level has 2-D tiles, GnTiling::t2d) pick the kernel instance.
void launch_track_gn(const GnArgs& a, int n_seq, int ppt, int group, bool t2d, hipStream_t s, int grid_seqs = 0);
void launch_prep_ref(const PrepArgs& a, hipStream_t s);
// LDS-tiled variant: a.tiles_x/tiles_y/margin/nblk must be set (see gn_tile_geometry)
void launch_track_gn_tile(const GnArgs& a, int n_seq, int ppt, hipStream_t s);
inline void gn_tile_geometry(int w, int h, int ppt, int& tiles_x, int& tiles_y)
{
    tiles_x = (w + 63) / 64;
    tiles_y = (h + 4 * ppt - 1) / (4 * ppt);
}
void launch_gn_solve(const SolveArgs& a, int n_seq, hipStream_t s);
// The opt-in terms of a launch pair.  `on` is the set of Term bits that are on -- robust weights count as
// TERM_ROBUST with the adaptive or a given scale and as TERM_MEDIAN with the median scale -- and the block of every term that is on is
// filled (the median scale fills rob as well; every other block stays value-initialised: rob.table == nullptr is "no robust weights"
// to the affine kernels).  The two launchers hold the table "set of terms -> kernel pair" once each: nothing on and TERM_STEP_CONTROL
// run the plain tile kernel (launch_track_gn: the mask stays), every other pair has no mask; false, and nothing launched, for a set
// without a kernel pair (Tracker::refusal lets none through).
enum Term : unsigned { TERM_ROBUST = 1, TERM_MEDIAN = 2, TERM_AFFINE = 4, TERM_GEOMETRIC = 8, TERM_STEP_CONTROL = 16 };
struct TileTerms  { unsigned on; RobustGn rob; MedianGn med; AffineGn aff; GeoGn geo; };
struct SolveTerms { unsigned on; RobustSolve rob; MedianSolve med; AffineSolve aff; GeoSolve geo; LmSolve lm; };
bool launch_track_gn_terms(const GnArgs& a, const TileTerms& t, int n_seq, int ppt, int group, bool t2d, hipStream_t s, int grid_seqs = 0);
bool launch_gn_solve_terms(const SolveArgs& a, const SolveTerms& t, int n_seq, hipStream_t s);
// one Tracker::track iteration in one launch for a few sequences (k_track_gn_fused); false = no instance for (ppt, group)
bool launch_track_gn_fused(const GnArgs& a, const SolveArgs& sa, int n_seq, int ppt, int group, bool t2d, int* ticket, int* report,
                           int* progress, hipStream_t s);
bool gn_fused_available(int ppt, int group);
// k_track_level: every iteration of one level in one launch (one workgroup per sequence); the level must have been
// tiled with raster tiles of 4 pixels per thread (ga.nblk = gn_blocks_per_seq(w, h, 4)) and have at most DVO_FUSED_MAX_TILES tiles
#define DVO_FUSED_MAX_TILES 8
void launch_track_level(const GnArgs& ga, const SolveArgs& sa, int n_seq, hipStream_t s);
void launch_track_begin(SeqState* state, dvo_track_log* log, int n_seq, int levels, hipStream_t s);
void launch_set_pose(SeqState* state, const float* xi_dev, int n_seq, hipStream_t s);
void launch_export_poses(const SeqState* state, float* xi_out, float* T_out, int n_seq, hipStream_t s, float* host_result = nullptr, int host_tag = 0);
void launch_se3(int op, const float* a, const float* b, float* out, hipStream_t s);
// k_pose_algebra: doubles per case that op reads and writes (include/dvo.h, dvo_op_pose_algebra); false for an unknown op
#define DVO_POSE_ALGEBRA_OPS 6
DVO_HD bool pose_algebra_row(int op, int& n_in, int& n_out)
{
    switch (op) {
    case 0: n_in = 6; n_out = 12; return true;
    case 1: n_in = 12; n_out = 6; return true;
    case 2: n_in = 12; n_out = 6; return true;
    case 3: n_in = 12; n_out = 31; return true;
    case 4: n_in = 27; n_out = 7; return true;
    case 5: n_in = 21; n_out = 42; return true;
    }
    n_in = 0; n_out = 0;
    return false;
}
void launch_pose_algebra(int op, int n, const double* in, double* out, hipStream_t s);
void launch_propagate(const float* ref_depth, const float* ref_sigma, const float* ref_age, int w, int h, const Intr& k,
                      const Pose& pose, float tz, int* owner, float* depth, float* sigma, float* age, hipStream_t s);
void launch_regularize(const float* depth, const float* sigma, int w, int h, float* out, hipStream_t s);
void launch_depth_update(const UpdateArgs& a, hipStream_t s);
void launch_ingest(const uint8_t* rgb, int channels, const uint16_t* depth16, int n, float depth_scale, float sigma_valid,
                   float sigma_invalid, int invalidate_gray, float* gray, float* depth, float* sigma, hipStream_t s);
void launch_selftest_trig(unsigned n, unsigned side, unsigned long long* out3, hipStream_t s);   // out3 = bits of the largest relative differences (sin, cos, atan2), pre-set 0
void launch_selftest_sqrt(unsigned long long* out3, hipStream_t s);          // out3 = {inputs, mismatches, first bad pattern}, pre-set {0, 0, ~0}
void launch_selftest_division(unsigned b_first, unsigned b_stride, unsigned b_count, unsigned long long* out3, hipStream_t s);   // (at most 2^17 values of b per launch)
void launch_selftest_reciprocal(unsigned long long* out3, hipStream_t s);  // out3 = {fast-path inputs, mismatches, first bad pattern}, pre-set {0, 0, ~0}
void launch_visualize(int mode, const float* a, const float* b, int n, uint8_t* rgb, hipStream_t s);
void launch_undistort(const float* src, int w, int h, const Intr& k, const float D[5], float border, float* dst, hipStream_t s);
// k_undistort_map: table[c][y][x] = undistort_source((x, y) << culls) of camera c (full-resolution w x h), tw x th top-level pixels
void launch_undistort_map(const UndistortCam* cams_dev, int n_cam, int w, int h, int culls, int tw, int th, int* table, hipStream_t s);

}  // namespace dvo
