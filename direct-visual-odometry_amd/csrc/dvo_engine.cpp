// dvo_engine.cpp -- host side of libdvo.so (see dvo_engine.h).  Reference citations: file:line under the reference tree.
#include "dvo_engine.h"

#include <hip/hip_runtime.h>

#include <array>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <utility>

#include <dlfcn.h>

namespace dvo {

// ------------------------------------------------------------------------------------------------ errors
static thread_local std::string g_error;
void set_error(const std::string& s) { g_error = s; }
const char* last_error() { return g_error.c_str(); }

int check_hip(hipError_t e, const char* what)
{
    if (e == hipSuccess) return DVO_OK;
    set_error(std::string(what) + ": " + hipGetErrorString(e));
    if (e == hipErrorNoDevice || e == hipErrorInvalidDevice) return DVO_ERR_NO_DEVICE;
    if (e == hipErrorOutOfMemory) return DVO_ERR_OUT_OF_MEMORY;
    return DVO_ERR_HIP;
}

// ------------------------------------------------------------------------------------------------ tracing (roctx, optional)
namespace {
struct Roctx {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    Roctx()
    {
        const char* e = getenv("DVO_TRACE");
        if (!e || e[0] == '0') return;
        // rocprofv3 (--marker-trace) intercepts the rocprofiler-sdk flavour of roctx; the legacy libroctx64 serves roctracer tools
        void* h = nullptr;
        for (const char* name : {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"}) {
            h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (h) break;
        }
        if (!h) return;
        push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
        pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
        if (!push || !pop) { push = nullptr; pop = nullptr; }
    }
};
Roctx& roctx() { static Roctx r; return r; }
}  // namespace
void trace_push(const char* name) { if (roctx().push) (void)roctx().push(name); }
void trace_pop() { if (roctx().pop) (void)roctx().pop(); }

bool host_buffer_is_pinned(const void* p)
{
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof at);
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();   // (an ordinary malloc'ed pointer is "invalid value" to HIP: not an error of ours)
        return false;
    }
    return at.type == hipMemoryTypeHost;
}

int select_device(int device)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        set_error("no HIP device visible: libdvo has no CPU fallback");
        return DVO_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= n) {
        set_error("device ordinal out of range");
        return DVO_ERR_BAD_ARGUMENT;
    }
    DVO_HIP(hipSetDevice(device));
    return DVO_OK;
}

int DevBuf::alloc(size_t n)
{
    release();
    if (n == 0) n = 4;
    DVO_HIP(hipMalloc(&p, n));
    bytes = n;
    return DVO_OK;
}
void DevBuf::release()
{
    if (p && owned) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
    owned = true;
}

int KeyframePool::take(size_t bytes, void** out)
{
    if (block_bytes == 0) block_bytes = (bytes + 255) & ~(size_t)255;
    if (bytes > block_bytes) { set_error("keyframe pool: block size changed"); return DVO_ERR_BAD_ARGUMENT; }
    if (free_blocks.empty()) {
        const int per_slab = 16;
        auto slab = std::make_unique<DevBuf>();
        DVO_TRY(slab->alloc(block_bytes * per_slab));
        for (int i = per_slab - 1; i >= 0; i--) free_blocks.push_back(static_cast<char*>(slab->p) + block_bytes * (size_t)i);
        slabs.push_back(std::move(slab));
    }
    *out = free_blocks.back();
    free_blocks.pop_back();
    return DVO_OK;
}

// ------------------------------------------------------------------------------------------------ geometry
static void cull_intrinsic(const float K[9], int times, float out[9])
{  // Convert::cullIntrinsic, convert.cpp:22-29
    if (times == 0) {
        memcpy(out, K, 9 * sizeof(float));
        return;
    }
    const double r = (double)(1 << times);
    for (int i = 0; i < 9; i++) out[i] = (float)((double)K[i] / r);
    out[8] = 1.0f;
}

int make_geometry(const float K[9], int w, int h, int levels, int culls, Geometry& g)
{
    if (levels < 1 || levels > DVO_MAX_LEVELS || culls < 0 || culls > 8 || w <= 0 || h <= 0) {
        set_error("bad pyramid geometry");
        return DVO_ERR_BAD_ARGUMENT;
    }
    g.src_w = w; g.src_h = h; g.levels = levels; g.culls = culls;
    const int bw = w >> culls, bh = h >> culls;
    float Kb[9];
    cull_intrinsic(K, culls, Kb);
    g.px_total = 0;
    for (int i = 0; i < levels; i++) {
        const int t = levels - 1 - i;  // frame.cpp:33-35
        g.w[i] = bw >> t; g.h[i] = bh >> t;
        if (g.w[i] < 4 || g.h[i] < 4) {  // k_track_gn's lanes without an interior position gather around (1, 1): rows / columns 0..3
            set_error("image too small for this many pyramid levels (every level must be at least 4 x 4)");
            return DVO_ERR_BAD_ARGUMENT;
        }
        if ((size_t)g.w[i] * g.h[i] >= (1u << 24)) {
            set_error("pyramid level larger than 2^24 pixels");
            return DVO_ERR_BAD_ARGUMENT;
        }
        cull_intrinsic(Kb, t, g.K9[i]);
        g.k[i] = make_intr(g.K9[i]);
        g.px_total += (size_t)g.w[i] * g.h[i];
    }
    return DVO_OK;
}

void level_intrinsics(const float K[9], const Geometry& g, Intr out[DVO_MAX_LEVELS], float (*K9_out)[9])
{   // make_geometry's steps, in its order: cull to the pyramid base, then to each level
    float Kb[9], Kl[9];
    cull_intrinsic(K, g.culls, Kb);
    for (int i = 0; i < g.levels; i++) {
        cull_intrinsic(Kb, g.levels - 1 - i, Kl);
        out[i] = make_intr(Kl);
        if (K9_out) memcpy(K9_out[i], Kl, sizeof Kl);
    }
}

int check_intrinsics(const char* who, const float* K, size_t n)
{
    if (!K) { set_error(std::string(who) + ": K is NULL"); return DVO_ERR_BAD_ARGUMENT; }
    for (size_t q = 0; q < n; q++) {
        const float* k = K + q * 9;
        for (int i = 0; i < 9; i++)
            if (!std::isfinite(k[i])) { set_error(std::string(who) + ": sequence " + std::to_string(q) + ": K has a non-finite entry"); return DVO_ERR_BAD_ARGUMENT; }
        if (!(k[0] > 0.0f) || !(k[4] > 0.0f)) { set_error(std::string(who) + ": sequence " + std::to_string(q) + ": fx and fy must be > 0"); return DVO_ERR_BAD_ARGUMENT; }
    }
    return DVO_OK;
}

static float level_step(const dvo_config& c, int level)
{  // optimize.cpp:22-26
    if (level == 1) return c.step_level1;
    if (level == 2) return c.step_level2;
    return c.step_default;
}

int FrameSet::alloc(const Geometry& geo, int n, const dvo_config& cfg, void* mem)
{
    g = geo;
    n_seq = n;
    if (mem) arena.adopt(mem, arena_bytes(g, n));
    else DVO_TRY(arena.alloc(arena_bytes(g, n)));
    float* p = arena.as<float>();
    for (int m = 0; m < 4; m++)
        for (int l = 0; l < g.levels; l++) {
            (m == 0 ? gray : m == 1 ? depth : m == 2 ? sigma : wgt)[l] = p;
            p += (size_t)g.w[l] * g.h[l] * n;
        }
    for (int l = 0; l < g.levels; l++) step[l] = level_step(cfg, l);
    sigma_min = cfg.sigma_min;
    sigma_max = cfg.sigma_max;
    allow_const_weight = cfg.min_depth > 0.0f && getenv("DVO_WEIGHT_MAPS") == nullptr;   // (the variable forces the maps: A/B runs, tests)
    return DVO_OK;
}

// wgt of every level from the current sigma pyramid (k_prep_ref)
static void prep_reference(FrameSet& fs, hipStream_t s)
{
    PrepArgs a{};
    a.depth = fs.depth[0]; a.sigma = fs.sigma[0]; a.wgt = fs.wgt[0];  // levels are contiguous
    size_t end = 0;
    for (int l = 0; l < fs.g.levels; l++) {
        end += (size_t)fs.g.w[l] * fs.g.h[l] * fs.n_seq;
        a.level_end[l] = end;
        a.step[l] = fs.step[l];
    }
    a.sigma_min = fs.sigma_min; a.sigma_max = fs.sigma_max;
    a.levels = fs.g.levels;
    launch_prep_ref(a, s);
}

static void fuse_prep(PyramidArgs& a, const FrameSet& fs)
{
    for (int l = 0; l < fs.g.levels; l++) {
        a.wgt[l] = fs.wgt[l];
        a.step[l] = fs.step[l];
    }
    a.sigma_min = fs.sigma_min; a.sigma_max = fs.sigma_max;
}

static void plan_copy(PyramidArgs& a, const uint8_t* seq_action, const FrameSet* from)
{
    if (!seq_action || !from) return;
    a.seq_action = seq_action;
    for (int l = 0; l < from->g.levels; l++) {
        a.ref[0][l] = from->gray[l]; a.ref[1][l] = from->depth[l]; a.ref[2][l] = from->sigma[l];
        a.ref_wgt[l] = from->wgt[l];
    }
}

// the geometry of a build from input frames: input size, the pyramid's levels and the rows the input buffers hold (everything else zero)
static PyramidArgs frame_args(const FrameSet& fs, bool rows_decimated)
{
    PyramidArgs a{};
    a.src_w = fs.g.src_w; a.src_h = fs.g.src_h; a.culls = fs.g.culls; a.levels = fs.g.levels;
    a.src_img_rows = rows_decimated ? fs.g.src_h >> fs.g.culls : fs.g.src_h;
    a.src_row_shift = rows_decimated ? 0 : fs.g.culls;
    for (int l = 0; l < fs.g.levels; l++) { a.w[l] = fs.g.w[l]; a.h[l] = fs.g.h[l]; }
    a.inv_tw = 1.0f / (float)fs.g.w[fs.g.top()];
    return a;
}

// the gray side of a build from raw frames: the bytes, their channel count, k_ingest's scale and the gray pyramid they go to
static PyramidArgs raw_gray_args(const FrameSet& fs, const FrameInput& in, bool rows_decimated)
{
    PyramidArgs a = frame_args(fs, rows_decimated);
    a.raw_rgb = in.rgb; a.raw_channels = in.channels; a.raw_gray_scale = (float)(1.0 / 255.0);
    for (int l = 0; l < fs.g.levels; l++) a.dst[0][l] = fs.gray[l];
    return a;
}

// the arguments of a build from float maps (the caller adds the plan's copy-forward and, optionally, the remap)
static PyramidArgs float_args(FrameSet& fs, const float* gray_dev, const float* depth_dev, const float* sigma_dev, bool keep_sigma,
                              bool rows_decimated)
{
    PyramidArgs a = frame_args(fs, rows_decimated);
    a.src[0] = gray_dev; a.src[1] = depth_dev; a.src[2] = sigma_dev;
    for (int l = 0; l < fs.g.levels; l++) {
        a.dst[0][l] = fs.gray[l]; a.dst[1][l] = fs.depth[l];
        a.dst[2][l] = (keep_sigma || !(depth_dev && sigma_dev)) ? fs.sigma[l] : nullptr;
    }
    fs.sigma_by_validity = false;
    if (depth_dev && sigma_dev) fuse_prep(a, fs);  // wgt written by the same launch (no k_prep_ref pass)
    return a;
}

void build_pyramid(FrameSet& fs, const float* gray_dev, const float* depth_dev, const float* sigma_dev, hipStream_t s, bool keep_sigma,
                   bool rows_decimated, const uint8_t* seq_action, const FrameSet* copy_from, PyramidKernel* ran)
{
    PyramidArgs a = float_args(fs, gray_dev, depth_dev, sigma_dev, keep_sigma, rows_decimated);
    plan_copy(a, seq_action, copy_from);
    const PyramidKernel k = launch_pyramid(a, fs.n_seq, s);
    if (ran) *ran = k;
}

bool build_pyramid(FrameSet& fs, const FrameInput& in, hipStream_t s, bool keep_sigma, const uint8_t* seq_action, const FrameSet* copy_from,
                   PyramidSplit* split, PyramidKernel* ran)
{
    PyramidKernel none;
    PyramidKernel& k = ran ? *ran : none;
    if (in.photo.gain) {   // raw mono frame of a calibrated handle (the callers refuse float frames): the k_pyramid*_photo kernels, gray
                           // only; with a remap whole frames and k_pyramid_remap_plan's SKIP, else k_pyramid's rows and copy-forward
        PyramidArgs a = raw_gray_args(fs, in, in.remap ? false : in.rows_decimated);
        a.remap = in.remap; a.remap_cam = in.remap_cam;
        if (in.remap) a.seq_action = seq_action;
        else plan_copy(a, seq_action, copy_from);
        fs.sigma_by_validity = false;
        k = launch_pyramid(a, fs.n_seq, s, &in.photo);
        return false;
    }
    if (in.remap && !in.has_depth()) {   // mono frame, lens undistortion fused in (k_pyramid_remap): gray only, whole frames
                                         // (a mono plan: k_pyramid_remap_plan, whose SKIP sequences write nothing; copy_from is not used)
        PyramidArgs a = raw_gray_args(fs, in, false);
        a.src[0] = in.gray;
        a.remap = in.remap; a.remap_cam = in.remap_cam;
        a.seq_action = seq_action;
        fs.sigma_by_validity = false;
        k = launch_pyramid(a, fs.n_seq, s);
        return false;
    }
    // sensor-depth frames with lens undistortion (dvo_batch_set_sensor_distortion): the arguments of the plain build plus the remap,
    // whole frames -- launch_pyramid picks k_pyramid_remap_depth
    if (!in.raw()) {
        if (!in.remap && !in.filter) { build_pyramid(fs, in.gray, in.depth, in.sigma, s, keep_sigma, in.rows_decimated, seq_action, copy_from, &k); return false; }
        PyramidArgs a = float_args(fs, in.gray, in.depth, in.sigma, keep_sigma, false);   // (remap or filter: whole frames)
        a.remap = in.remap; a.remap_cam = in.remap_cam;
        plan_copy(a, seq_action, copy_from);
        k = launch_pyramid(a, fs.n_seq, s, nullptr, in.filter);
        return false;
    }
    PyramidArgs a = raw_gray_args(fs, in, in.filter ? false : in.rows_decimated);
    a.raw_depth = in.depth16; a.raw_depth_scale = in.depth_scale;
    a.raw_sigma_valid = 0.1f; a.raw_sigma_invalid = 1.0f; a.raw_invalidate_gray = 1;   // transform.cpp:60-76
    const bool dep = in.depth16 != nullptr;
    for (int l = 0; l < fs.g.levels; l++) {
        a.dst[1][l] = dep ? fs.depth[l] : nullptr;
        a.dst[2][l] = (dep && keep_sigma) ? fs.sigma[l] : nullptr;
    }
    fs.sigma_by_validity = dep && !keep_sigma && fs.allow_const_weight;
    if (fs.sigma_by_validity) {  // no wgt maps: the weight of every pixel that can contribute is a constant of the level
        for (int l = 0; l < fs.g.levels; l++) fs.wgt_valid[l] = gn_weight(fs.step[l], fs.sigma_min, fs.sigma_max, a.raw_sigma_valid);
    } else if (dep) {
        fuse_prep(a, fs);
    }
    a.remap = in.remap; a.remap_cam = in.remap_cam;   // (set only with depth here, and then on whole frames)
    plan_copy(a, seq_action, copy_from);
    if (split && !in.filter && pyramid_can_split(a)) {
        // stage A where the single kernel would run; stage B on the side stream, after everything queued on `s` so far (every earlier
        // launch that may still read the set it overwrites)
        k = {DVO_PYRAMID_KERNEL_SPLIT, a.culls, 0};
        launch_pyramid_coarse(a, fs.n_seq, s);
        split->err = hipEventRecord(split->fork, s);
        if (split->err == hipSuccess) split->err = hipStreamWaitEvent(split->side, split->fork, 0);
        launch_pyramid_rest(a, fs.n_seq, split->err == hipSuccess ? split->side : s);
        if (split->err == hipSuccess) split->err = hipEventRecord(split->done, split->side);
        return split->err == hipSuccess;
    }
    k = launch_pyramid(a, fs.n_seq, s, nullptr, in.filter);
    return false;
}

int upload_rows(void* dst, const void* src, size_t row_bytes, int img_rows, size_t n_img, int culls, bool decimate, hipStream_t s,
                    size_t* stored)
{
    if (!decimate || culls <= 0) {
        const size_t n = row_bytes * (size_t)img_rows * n_img;
        if (stored) *stored = n;
        DVO_HIP(hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, s));
        return DVO_OK;
    }
    // img_rows is a multiple of 2^culls (can_decimate_rows), so the kept rows of ALL images are the rows r = 0 (mod 2^culls) of the
    // n_img * img_rows rows of the whole buffer: one 2-D copy with a source pitch of 2^culls rows
    const size_t rows = ((size_t)img_rows >> culls) * n_img;
    if (stored) *stored = row_bytes * rows;
    DVO_HIP(hipMemcpy2DAsync(dst, row_bytes, src, row_bytes << culls, row_bytes, rows, hipMemcpyHostToDevice, s));
    return DVO_OK;
}

int Photometry::set(const char* who, int n, const float* resp, const float* vign, const int* cal_of_seq, int n_seq, const Geometry& g,
                    const Undistortion& und, hipStream_t s)
{
    if (n < 0) { set_error(std::string(who) + ": n_cal is negative"); return DVO_ERR_BAD_ARGUMENT; }
    if (n > 0 && !resp && !vign) { set_error(std::string(who) + ": n_cal > 0 needs inv_response, vignette or both"); return DVO_ERR_BAD_ARGUMENT; }
    if (resp)
        for (int c = 0; c < n; c++)
            for (int i = 0; i < 256; i++) {
                const float v = resp[(size_t)c * 256 + i];
                if (!std::isfinite(v) || v < 0.0f) {
                    set_error(std::string(who) + ": inv_response entry " + std::to_string(i) + " of calibration " + std::to_string(c) +
                              " is not finite or is negative");
                    return DVO_ERR_BAD_ARGUMENT;
                }
            }
    if (cal_of_seq && n > 0)
        for (int q = 0; q < n_seq; q++)
            if (cal_of_seq[q] < 0 || cal_of_seq[q] >= n) {
                set_error(std::string(who) + ": seq_cal of sequence " + std::to_string(q) + " is " + std::to_string(cal_of_seq[q]) +
                          ", outside [0, " + std::to_string(n) + ")");
                return DVO_ERR_BAD_ARGUMENT;
            }
    DVO_HIP(hipStreamSynchronize(s));   // (the previous tables may still be read by queued work: none before the first frame)
    clear();
    if (n == 0) return DVO_OK;
    const size_t px = (size_t)g.src_w * g.src_h;
    response.resize((size_t)n * 256);
    for (int c = 0; c < n; c++)
        for (int i = 0; i < 256; i++) response[(size_t)c * 256 + i] = resp ? resp[(size_t)c * 256 + i] : (float)i * (float)(1.0 / 255.0);
    if (vign) vignette.assign(vign, vign + px * (size_t)n);
    seq_cal.assign((size_t)n_seq, 0);
    if (cal_of_seq) seq_cal.assign(cal_of_seq, cal_of_seq + n_seq);
    n_cal = n;
    const int rc = rebuild(n_seq, g, und, s);
    if (rc != DVO_OK) clear();   // (no calibration rather than a half-built one)
    return rc;
}

int Photometry::rebuild(int n_seq, const Geometry& g, const Undistortion& und, hipStream_t s)
{
    if (!enabled()) return DVO_OK;
    // one gain table per distinct (calibration, undistortion camera): the integer pair, not the table's contents
    std::map<std::pair<int, int>, int> ids;
    std::vector<int> pairs;
    seq_pair.assign((size_t)n_seq, 0);
    for (int q = 0; q < n_seq; q++) {
        const std::pair<int, int> key(seq_cal[(size_t)q], und.enabled() ? und.cam_of[(size_t)q] : 0);
        auto it = ids.emplace(key, (int)ids.size());
        if (it.second) { pairs.push_back(key.first); pairs.push_back(key.second); }
        seq_pair[(size_t)q] = it.first->second;
    }
    n_pair = (int)ids.size();
    const int T = g.top(), tw = g.w[T], th = g.h[T];
    const size_t head = ((size_t)n_seq + 3) & ~(size_t)3;
    DevBuf pairs_dev, vign_dev;
    DVO_TRY(pairs_dev.alloc(sizeof(int) * pairs.size()));
    if (!vignette.empty()) DVO_TRY(vign_dev.alloc(sizeof(float) * vignette.size()));
    DVO_HIP(hipStreamSynchronize(s));
    DVO_TRY(resp_dev.alloc(sizeof(float) * response.size()));
    DVO_TRY(idx_dev.alloc(sizeof(int) * 2 * head));
    DVO_TRY(gain_dev.alloc(sizeof(float) * (size_t)n_pair * tw * th));
    DVO_HIP(hipMemcpyAsync(resp_dev.p, response.data(), sizeof(float) * response.size(), hipMemcpyHostToDevice, s));
    DVO_HIP(hipMemsetAsync(idx_dev.p, 0, idx_dev.bytes, s));
    DVO_HIP(hipMemcpyAsync(idx_dev.p, seq_cal.data(), sizeof(int) * (size_t)n_seq, hipMemcpyHostToDevice, s));
    DVO_HIP(hipMemcpyAsync(idx_dev.as<int>() + head, seq_pair.data(), sizeof(int) * (size_t)n_seq, hipMemcpyHostToDevice, s));
    DVO_HIP(hipMemcpyAsync(pairs_dev.p, pairs.data(), pairs_dev.bytes, hipMemcpyHostToDevice, s));
    if (vign_dev.p) DVO_HIP(hipMemcpyAsync(vign_dev.p, vignette.data(), vign_dev.bytes, hipMemcpyHostToDevice, s));
    launch_photometric_map(vign_dev.as<float>(), pairs_dev.as<int>(), n_pair, g.src_w, g.src_h, g.culls, tw, th,
                           und.enabled() ? und.table(n_seq) : nullptr, gain_dev.as<float>(), s);
    DVO_HIP(hipGetLastError());
    DVO_HIP(hipStreamSynchronize(s));   // (pairs_dev and vign_dev go out of scope)
    return DVO_OK;
}

void redecimate(FrameSet& fs, const float* depth_top, const float* sigma_top, hipStream_t s)
{  // level i = cullImage(top, levels-1-i); the top level itself is the map handed in (frame.cpp:39-61)
    PyramidArgs a{};
    const int T = fs.g.top();
    a.src[1] = depth_top; a.src[2] = sigma_top;
    a.src_w = fs.g.w[T]; a.src_h = fs.g.h[T]; a.levels = fs.g.levels;
    a.src_img_rows = a.src_h;
    fs.sigma_by_validity = false;
    for (int l = 0; l < fs.g.levels; l++) {
        a.w[l] = fs.g.w[l]; a.h[l] = fs.g.h[l];
        a.dst[1][l] = fs.depth[l]; a.dst[2][l] = fs.sigma[l];
    }
    a.inv_tw = 1.0f / (float)fs.g.w[T];
    if (depth_top && sigma_top) fuse_prep(a, fs);
    launch_pyramid(a, fs.n_seq, s);
    if (!(depth_top && sigma_top)) prep_reference(fs, s);  // one map only: the other comes from the stored pyramid
}

// ------------------------------------------------------------------------------------------------ tracker
Tracker::~Tracker()
{
    if (h_state) (void)hipHostFree(h_state);
    if (h_progress) (void)hipHostFree(h_progress);
    if (h_result) (void)hipHostFree(h_result);
    for (auto st : sub_streams) (void)hipStreamDestroy(st);
    for (auto e : ev_join) (void)hipEventDestroy(e);
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    for (auto& e : ev_pool) {
        (void)hipEventDestroy(e.first);
        (void)hipEventDestroy(e.second);
    }
}

int Tracker::init(const Geometry& geo, int n, const dvo_config& c)
{
    g = geo; n_seq = n; cfg = c;
    if (cfg.max_iterations < 1 || cfg.max_iterations > DVO_MAX_ITERATIONS || cfg.fixed_iterations > DVO_MAX_ITERATIONS) {
        set_error("iteration counts must be within [1, DVO_MAX_ITERATIONS]");
        return DVO_ERR_BAD_ARGUMENT;
    }
    for (int l = 0; l < g.levels; l++)
        if (g.w[l] < 4 || g.h[l] < 4) {  // k_track_gn's parked lanes gather the 4 x 4 taps around (1, 1): every level must hold them
            set_error("pyramid level smaller than 4 x 4 pixels");
            return DVO_ERR_BAD_ARGUMENT;
        }
    if ((unsigned long long)n_seq * (unsigned long long)g.w[g.top()] * g.h[g.top()] / 256ull >= (1ull << 31)) {
        set_error("too many sequences for one launch grid");
        return DVO_ERR_BAD_ARGUMENT;
    }
    size_t max_part = 0;
    // gn_use_lds_patch: -1 = auto, 0 = global gathers, N > 0 = LDS patch with margin N.  Auto is the global-gather
    // kernel: measured on MI355X (profiles/r01_gn_variants.md) the LDS-staged variant is 10-15 % slower.
    // The configured margin decides n_sub, adaptive, DVO_PLAN_ITERATION and persist_ok below for the handle's whole life, whichever
    // plan is in force later; a level's own margin (LevelPlan::margin) is what its launches use.
    const int margin = cfg.gn_use_lds_patch < 0 ? 0 : (cfg.gn_use_lds_patch > 24 ? 24 : cfg.gn_use_lds_patch);
    // robust: the weighted plan (lv_rw) -- the global-gather kernel, no fused level, the batch tiling
    auto plan_level = [&](int l, bool robust) -> LevelPlan {
        LevelPlan L{};
        int p = cfg.gn_pixels_per_thread;
        const bool auto_p = (p != 1 && p != 2 && p != 4 && p != 8);
        if (auto_p) p = 4;  // auto: biggest tile that still gives >= 4 workgroups per CU
        if (margin > 0 && !robust) {
            L.schedule = DVO_PLAN_LDS_PATCH; L.margin = margin;
            gn_tile_geometry(g.w[l], g.h[l], p, L.tiles_x, L.tiles_y);
            while (auto_p && p > 1 && (size_t)n_seq * L.tiles_x * L.tiles_y < 1024) {
                p >>= 1;
                gn_tile_geometry(g.w[l], g.h[l], p, L.tiles_x, L.tiles_y);
            }
            L.nblk = L.tiles_x * L.tiles_y;
        } else {
            // small levels: every iteration inside one k_track_level launch (tiles of 256 x 4 pixels)
            // Off by default: measured on MI355X (512 sequences) the one-workgroup-per-sequence form runs the two coarse
            // levels in ~1.0 ms against ~0.6 ms for the batched launches -- 2 waves per SIMD cannot hide the latency chain
            // of a tile, while the batched kernels share the whole chip among the sequences that are still active.
            const int fuse_max = (cfg.track_fused_tiles <= 0 || robust) ? 0
                                                            : (cfg.track_fused_tiles > DVO_FUSED_MAX_TILES ? DVO_FUSED_MAX_TILES : cfg.track_fused_tiles);
            const int crop_l = level_params(l).crop;
            const GnTiling t4 = gn_tiling(g.w[l], g.h[l], 4, crop_l);
            const bool fused = fuse_max > 0 && !t4.t2d && t4.count <= fuse_max;  // (k_track_level: raster tiles)
            L.schedule = fused ? DVO_PLAN_LEVEL : DVO_PLAN_PAIRS;
            if (fused) p = 4;
            // (one sequence on the one-launch-per-call schedule keeps 4 pixels per thread: k_track_persist's workgroups wait for each
            //  other, and 75 of them hand over faster than 300 -- 406 against 451 us per 640x480 frame, profiles/r03_single_ab.txt)
            //  A mono handle's levels (at most 160 x 120) show no such difference -- 132-140 us per frame at 1, 2 and 4 pixels per
            //  thread -- so it keeps the tile size every other schedule picks for one sequence (persist_ppt < 0): the same bits.)
            const bool single_p4 = !robust && prefer_persist && n_seq == 1 && cfg.track_single_launch == 0 && !cfg.profile && persist_ppt >= 0;
            if (single_p4 && auto_p && persist_ppt > 0) p = persist_ppt;
            while (!fused && auto_p && !single_p4 && p > 1 && (size_t)n_seq * gn_blocks_per_seq(g.w[l], g.h[l], p, crop_l) < 1024) p >>= 1;
            L.tiling = gn_tiling(g.w[l], g.h[l], p, crop_l);   // the level's tiles are decided: every launch takes them from here
            L.nblk = L.tiling.count;
        }
        L.ppt = p;
        int gg = cfg.gn_gather_group;
        if (gg != 1 && gg != 2 && gg != 4) gg = 2;
        while (gg > p || p % gg) gg >>= 1;
        L.group = gg < 1 ? 1 : gg;
        if ((size_t)L.nblk > max_part) max_part = L.nblk;
        return L;
    };
    for (int l = 0; l < g.levels; l++) {
        lv[l] = plan_level(l, false);
        lv_rw[l] = plan_level(l, true);
    }
    DVO_TRY(state.alloc(sizeof(SeqState) * (size_t)n_seq));
    part_rows = max_part;
    DVO_TRY(partials.alloc(sizeof(float) * 32 * max_part * (size_t)n_seq));
    DVO_TRY(log.alloc(sizeof(dvo_track_log) * (size_t)n_seq));
    DVO_TRY(counters.alloc(2 * sizeof(unsigned long long)));
    // sub-batches on concurrent streams: only for the sync-free schedule of big batches (the small-batch poll needs one chain)
    n_sub = cfg.track_streams;
    if (n_sub <= 0) n_sub = 1;
    if (n_sub > 8) n_sub = 8;
    if (n_seq <= 8 || margin > 0) n_sub = 1;
    while (n_sub > 1 && n_seq / n_sub < 8) n_sub--;
    for (int k = 1; k < n_sub; k++) {
        hipStream_t st = nullptr;
        hipEvent_t ev = nullptr;
        DVO_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        sub_streams.push_back(st);
        DVO_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        ev_join.push_back(ev);
    }
    if (n_sub > 1) DVO_HIP(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
    DVO_TRY(work.alloc(2 * sizeof(int) * (size_t)n_sub * (size_t)(n_seq + 4)));
    DVO_HIP(hipMemset(work.p, 0, work.bytes));
    // adaptive schedule (see dvo_engine.h): one launch chain only, global-gather kernel only, reference stop tests only
    adaptive = cfg.track_adaptive >= 0 && n_sub == 1 && margin == 0 && cfg.fixed_iterations <= 0;
    if (adaptive) {
        const size_t words = 2 * (size_t)DVO_MAX_LEVELS * DVO_MAX_ITERATIONS;
        // fine-grained (coherent) host memory: the device publishes a word with a system-scope release store and the host
        // sees it without waiting for a kernel boundary (coarse-grained memory only guarantees that after a host sync)
        DVO_HIP(hipHostMalloc(reinterpret_cast<void**>(&h_progress), words * sizeof(int), hipHostMallocMapped | hipHostMallocCoherent));
        memset(h_progress, 0, words * sizeof(int));
        DVO_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&d_progress), h_progress, 0));
    }
    // one launch per iteration (k_track_gn_fused) for handles of a few sequences, per level: the kernel carries the solve's 248
    // VGPRs (two waves per SIMD), so only where the level's grid is a few dozen workgroups -- measured on one 640x480 stream:
    // 14-16 us per iteration against 17-18 us for the launch pair up to 52 workgroups, but 31 us against 18 us at 300
    for (int l = 0; l < g.levels; l++) {
        LevelPlan& L = lv[l];
        if (cfg.track_single_launch >= 0 && n_seq <= 8 && margin == 0 && L.schedule == DVO_PLAN_PAIRS && !cfg.profile && n_sub == 1 &&
            gn_fused_available(L.ppt, L.group) && L.tiling.live_count > 0 && (long long)n_seq * L.tiling.live_count <= 64)
            L.schedule = DVO_PLAN_ITERATION;
    }
    for (int l = 0; l < DVO_MAX_LEVELS; l++) lv_plain[l] = lv[l];
    // ~0.2 s of polling per wait: far beyond any iteration, short enough that a wedged launch ends.  DVO_PERSIST_SPIN_LIMIT (tests): a
    // limit of 0 makes every launch give up at once, so the fallback path runs; DVO_PERSIST_TIMELINE: in-kernel stamps (diagnostic).
    persist_spin_limit = 1 << 18;
    if (const char* e = getenv("DVO_PERSIST_SPIN_LIMIT")) persist_spin_limit = atoi(e);
    if (const char* e = getenv("DVO_PERSIST_TIMELINE")) { persist_timeline = true; persist_dbg_worker = atoi(e); }
    // k_track_persist (one launch per track() call): one sequence, the global-gather kernel, one (ppt, group) pair on every level,
    // every level within the wide reduction's row limit, no profiling; track_single_launch: < 0 = launch pairs only, 1 = one launch per
    // iteration at most (k_track_gn_fused), 0 (default) = one launch per call where the result goes through enable_host_result().
    // This is the handle's half of the decision; persist_call() adds the call's.
    persist_ok = prefer_persist && n_seq == 1 && margin == 0 && !cfg.profile && cfg.track_single_launch == 0 && n_sub == 1 && track_persist_available(lv[0].ppt, lv[0].group);
    int max_tiles = 0;
    for (int l = 0; l < g.levels && persist_ok; l++) {
        const GnTiling& tl = lv[l].tiling;
        if (lv[l].ppt != lv[0].ppt || lv[l].group != lv[0].group || lv[l].schedule == DVO_PLAN_LEVEL || lv[l].nblk > 320 || tl.live_count <= 0) persist_ok = false;
        if (tl.live_count > max_tiles) max_tiles = tl.live_count;
    }
    if (persist_ok) {
        int cap = 0;
        if (track_persist_max_grid(lv[0].ppt, lv[0].group, &cap) != DVO_OK || cap < 1) persist_ok = false;
        else {
            persist_grid = 1 + (max_tiles < cap - 1 ? max_tiles : cap - 1);   // the solver + one worker per tile of the largest level, all resident at once (they wait for each other)
            DVO_TRY(persist_ctl.alloc((16 + (size_t)persist_grid) * sizeof(int)));   // control line (64 B) + one arrival slot per workgroup
            DVO_HIP(hipMemset(persist_ctl.p, 0, persist_ctl.bytes));
        }
    }
    DVO_TRY(ticket.alloc(sizeof(int) * (size_t)n_seq));
    DVO_HIP(hipMemset(ticket.p, 0, ticket.bytes));
    DVO_TRY(freport.alloc(sizeof(int) * 2 * 2 * (size_t)DVO_MAX_LEVELS * DVO_MAX_ITERATIONS));
    DVO_HIP(hipMemset(freport.p, 0, freport.bytes));
    DVO_TRY(xi_out.alloc(sizeof(float) * 6 * (size_t)n_seq));
    DVO_TRY(T_out.alloc(sizeof(float) * 16 * (size_t)n_seq));
    DVO_HIP(hipMemset(counters.p, 0, 2 * sizeof(unsigned long long)));
    DVO_HIP(hipMemset(log.p, 0, log.bytes));
    return DVO_OK;
}

GnParams Tracker::level_params(int level) const
{
    GnParams p;
    p.step = cfg.step_default;  // optimize.cpp:22-26
    if (level == 1) p.step = cfg.step_level1;
    if (level == 2) p.step = cfg.step_level2;
    p.sigma_min = cfg.sigma_min; p.sigma_max = cfg.sigma_max;
    p.min_depth = cfg.min_depth;
    p.crop = (cfg.crop_enable && level == 2) ? 1 : 0;  // optimize.cpp:33-36
    return p;
}

GnArgs Tracker::gn_args(const float* obj_gray, const float* ref_gray, const float* ref_depth, const float* ref_wgt, float wgt_const, int level,
                        uint8_t* mask, int ignore_active) const
{
    const LevelPlan& L = lv[level];
    GnArgs a{};
    a.obj_gray = obj_gray;
    a.ref_gray = ref_gray;
    a.ref_depth = ref_depth;
    a.ref_wgt = ref_wgt;
    a.wgt_const = wgt_const;
    a.state = state.as<SeqState>();
    a.partials = partials.as<float>();
    a.mask = mask;
    a.w = g.w[level]; a.h = g.h[level]; a.nblk = L.nblk;
    a.inv_w = 1.0f / (float)g.w[level];
    a.q256 = 256 / g.w[level]; a.r256 = 256 % g.w[level];
    a.k = g.k[level];
    a.prm = level_params(level);
    a.ignore_active = ignore_active;
    // the level's tiles (k_track_gn_tile: L.tiling is the default, whose fields are the ones GnArgs starts with)
    a.blk_first = L.tiling.live_first; a.blk_count = L.tiling.live_count;
    a.t_shift = L.tiling.shift; a.x_org = L.tiling.x_org; a.y_org = L.tiling.y_org;
    a.tiles_x = L.tiling.t2d ? L.tiling.tiles_x : L.tiles_x; a.tiles_y = L.tiles_y; a.margin = L.margin;
    return a;
}

GnArgs Tracker::gn_args(const FrameSet& obj, const FrameSet& ref, int level, uint8_t* mask, int ignore_active) const
{
    return gn_args(obj.gray[level], ref.gray[level], ref.depth[level], ref.sigma_by_validity ? nullptr : ref.wgt[level],
                   ref.sigma_by_validity ? ref.wgt_valid[level] : 0.0f, level, mask, ignore_active);
}

SolveArgs Tracker::solve_args(int level, int q0, int ignore_active, SolveRows rows) const
{
    const GnTiling& tl = lv[level].tiling;
    SolveArgs a{};
    a.state = state.as<SeqState>() + q0;
    a.partials = partials.as<float>() + (size_t)q0 * part_rows * 32;   // (gn_view()'s partials of these sequences)
    a.log = log.as<dvo_track_log>() + q0;
    a.nblk = lv[level].nblk; a.level = level;
    // (profile counter: the pixels k_track_gn actually reads -- tiles outside the crop rows are never launched)
    a.level_pixels = rows == SolveRows::LivePair ? (int)tl.live_pixels : g.w[level] * g.h[level];
    if (rows != SolveRows::All) { a.blk_first = tl.live_first; a.blk_count = tl.live_count; }
    a.max_iterations = cfg.max_iterations; a.fixed_iterations = cfg.fixed_iterations;
    a.min_update = cfg.min_update; a.min_residual = cfg.min_residual;
    a.ignore_active = ignore_active;
    if (quality && level == g.levels - 1) a.result = quality + q0;   // (dvo_batch_set_track_quality: the finest level's solves)
    return a;
}

void Tracker::use_plan()
{
    const bool opt_in_term = terms_on() != 0;
    for (int l = 0; l < DVO_MAX_LEVELS; l++) lv[l] = opt_in_term ? lv_rw[l] : lv_plain[l];
}

SolveRows Tracker::pair_rows(int level, SolveRows live) const { return lv[level].schedule == DVO_PLAN_LDS_PATCH ? SolveRows::All : live; }

unsigned Tracker::terms_on() const
{
    return (rob.on ? (rob.median() ? TERM_MEDIAN : TERM_ROBUST) : 0u) | (aff.on ? TERM_AFFINE : 0u) | (geo.on ? TERM_GEOMETRIC : 0u) |
           (lm.on ? TERM_STEP_CONTROL : 0u);
}

const TermName* Tracker::refusal(unsigned on, TermSetter want)
{
    // the terms, in the order a refusal names them when several are on
    static const TermName kTerms[] = {{TERM_STEP_CONTROL, "step control is on", "dvo_batch_set_step_control"},
                                      {TERM_GEOMETRIC, "the geometric term is on", "dvo_batch_set_geometric"},
                                      {TERM_AFFINE, "affine brightness compensation is on", "dvo_batch_set_affine_brightness"},
                                      {TERM_MEDIAN, "the median robust scale is on", "dvo_batch_set_robust_median"},
                                      {TERM_ROBUST, "robust weights are on", "dvo_batch_set_robust_weights"}};
    // the table: the terms that refuse each setter's "on" call (a setter's own term never does: setting again reconfigures)
    unsigned refused_by = 0;
    switch (want) {
    case TermSetter::RobustWeights:    refused_by = TERM_STEP_CONTROL | TERM_GEOMETRIC; break;
    case TermSetter::RobustMedian:     refused_by = TERM_STEP_CONTROL | TERM_GEOMETRIC | TERM_AFFINE; break;
    case TermSetter::AffineBrightness: refused_by = TERM_STEP_CONTROL | TERM_GEOMETRIC | TERM_MEDIAN; break;
    case TermSetter::Geometric:        refused_by = TERM_STEP_CONTROL | TERM_AFFINE | TERM_MEDIAN | TERM_ROBUST; break;
    case TermSetter::GeometricAffine:  refused_by = TERM_STEP_CONTROL | TERM_MEDIAN | TERM_ROBUST; break;
    case TermSetter::StepControl:      refused_by = TERM_GEOMETRIC | TERM_AFFINE | TERM_MEDIAN | TERM_ROBUST; break;
    }
    for (const TermName& t : kTerms)
        if (on & refused_by & t.term) return &t;
    return nullptr;
}

template <class Apply> int Tracker::set_term(const char* who, TermSetter want, bool enable, Apply&& apply)
{
    if (enable)
        if (const TermName* t = refusal(terms_on(), want)) {
            set_error(std::string(who) + ": " + t->is_on + " (" + t->setter + "): the two do not combine");
            return DVO_ERR_BAD_ARGUMENT;
        }
    const int rc = apply();
    use_plan();
    return rc;
}

int HostRows::set(const float* rows, bool on_device, size_t bytes, hipStream_t s)
{
    if (!rows || on_device) { src = rows; return DVO_OK; }   // (device rows: read by the term's begin kernel in stream order)
    void* h = nullptr;
    DVO_TRY(stage.acquire(&h));
    memcpy(h, rows, bytes);
    DVO_TRY(stage.commit(dev.p, bytes, s));   // in stream order: after the begin kernel of every earlier push
    src = dev.as<float>();
    return DVO_OK;
}

int Tracker::log_iterations() const
{
    const int its = cfg.max_iterations > cfg.fixed_iterations ? cfg.max_iterations : cfg.fixed_iterations;
    return its > DVO_MAX_ITERATIONS ? DVO_MAX_ITERATIONS : (its < 1 ? 1 : its);
}

int Tracker::set_robust(const char* who, const dvo_robust_config* c, hipStream_t s)
{
    const bool enable = c && c->kind != DVO_ROBUST_NONE;
    const TermSetter want = enable && c->scale_mode == DVO_ROBUST_SCALE_MEDIAN ? TermSetter::RobustMedian : TermSetter::RobustWeights;
    return set_term(who, want, enable, [&] { return apply_robust(c, s); });
}

int Tracker::set_affine(const char* who, const dvo_affine_config* c, hipStream_t s)
{
    return set_term(who, TermSetter::AffineBrightness, c && c->mode != DVO_AFFINE_OFF, [&] { return apply_affine(c, s); });
}

int Tracker::set_geometric(const char* who, const dvo_geometric_config* c, hipStream_t s)
{
    return set_term(who, TermSetter::Geometric, c && c->mode != DVO_GEOMETRIC_OFF, [&] { return apply_geometric(c, s); });
}

int Tracker::set_geometric_affine(const char* who, const dvo_geometric_config* gc, const dvo_affine_config* ac, hipStream_t s)
{
    return set_term(who, TermSetter::GeometricAffine, true, [&] {
        DVO_TRY(apply_geometric(gc, s));
        return apply_affine(ac, s);
    });
}

int Tracker::set_step_control(const char* who, const dvo_lm_config* c, hipStream_t s)
{
    return set_term(who, TermSetter::StepControl, c && c->mode != DVO_LM_OFF, [&] { return apply_step_control(c, s); });
}

int Tracker::apply_robust(const dvo_robust_config* c, hipStream_t s)
{
    const bool enable = c && c->kind != DVO_ROBUST_NONE;
    if (enable && !rob.table.p) {
        DVO_TRY(rob.table.alloc(sizeof(RobustEntry) * (size_t)n_seq));
        DVO_TRY(rob.last.alloc(sizeof(float) * (size_t)n_seq));
        DVO_TRY(rob.scales.dev.alloc(sizeof(float) * (size_t)n_seq));
        DVO_TRY(rob.scales.stage.alloc(sizeof(float) * (size_t)n_seq));
        DVO_HIP(hipMemsetAsync(rob.last.p, 0, rob.last.bytes, s));
    }
    if (enable && c->scale_mode == DVO_ROBUST_SCALE_MEDIAN && !rob.hist.p) {
        rob.log_its = log_iterations();
        DVO_TRY(rob.hist.alloc(sizeof(uint32_t) * DVO_MEDIAN_BINS * (size_t)n_seq));
        DVO_TRY(rob.hist_last.alloc(sizeof(uint32_t) * DVO_MEDIAN_BINS * (size_t)n_seq));
        DVO_TRY(rob.mlog.alloc(sizeof(int) * 3 * (size_t)rob.log_its * (size_t)g.levels * (size_t)n_seq));
        DVO_TRY(rob.prime_mn.alloc(sizeof(int) * 2 * (size_t)n_seq));
        DVO_HIP(hipMemsetAsync(rob.hist.p, 0, rob.hist.bytes, s));
        DVO_HIP(hipMemsetAsync(rob.hist_last.p, 0, rob.hist_last.bytes, s));
        DVO_HIP(hipMemsetAsync(rob.mlog.p, 0, rob.mlog.bytes, s));
        DVO_HIP(hipMemsetAsync(rob.prime_mn.p, 0, rob.prime_mn.bytes, s));
    }
    rob.on = enable;
    if (enable) {
        if (rob.mode != c->scale_mode || c->scale_mode != DVO_ROBUST_SCALE_GIVEN) rob.scales.clear();   // (rows belong to one GIVEN configuration)
        rob.kind = c->kind; rob.mode = c->scale_mode; rob.param = c->param;
        rob.floor2 = c->scale_mode != DVO_ROBUST_SCALE_GIVEN ? c->scale_floor * c->scale_floor : 0.0f;
    } else {
        rob.scales.clear();
    }
    return DVO_OK;
}

template <class W, class Last, class Log, class Tracked, class Unpack>
int Tracker::read_term_log(const W* log_dev, int words, int log_its, int seq, const Last* last_dev, Log* out, hipStream_t s, Tracked tracked,
                           Unpack unpack, LogCopy extra, bool* did_track) const
{
    static_assert(sizeof(W) == 4, "a log is made of 4-byte words");
    std::vector<W> rows((size_t)words * log_its * g.levels);
    int n_iter[DVO_MAX_LEVELS] = {0};
    Last last{};
    DVO_HIP(hipMemcpyAsync(rows.data(), log_dev + (size_t)seq * rows.size(), sizeof(W) * rows.size(), hipMemcpyDeviceToHost, s));
    DVO_HIP(hipMemcpyAsync(n_iter, log.as<dvo_track_log>()[seq].n_iter, sizeof n_iter, hipMemcpyDeviceToHost, s));
    DVO_HIP(hipMemcpyAsync(&last, last_dev + seq, sizeof last, hipMemcpyDeviceToHost, s));
    if (extra.bytes) DVO_HIP(hipMemcpyAsync(extra.dst, extra.src, extra.bytes, hipMemcpyDeviceToHost, s));
    DVO_HIP(hipStreamSynchronize(s));
    const int size = out->struct_size;
    memset(out, 0, sizeof *out);
    out->struct_size = size;
    out->levels = g.levels;
    const bool did = tracked(last);   // else the sequence did not track at that push: an empty log
    if (did_track) *did_track = did;
    for (int l = 0; did && l < g.levels; l++) {
        const int n = n_iter[l] < log_its ? n_iter[l] : log_its;
        out->n_iter[l] = n;
        for (int it = 0; it < n; it++) unpack(l, it, &rows[((size_t)l * log_its + it) * words]);
    }
    return DVO_OK;
}

// device -> host on `s`, then the synchronize every read of a record ends with
static int read_back(void* dst, const void* src, size_t bytes, hipStream_t s)
{
    DVO_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s));
    DVO_HIP(hipStreamSynchronize(s));
    return DVO_OK;
}

int Tracker::last_robust_scales(float* s2, hipStream_t s) const { return read_back(s2, rob.last.p, sizeof(float) * (size_t)n_seq, s); }

int Tracker::last_robust_log(int seq, dvo_robust_log* out, hipStream_t s) const
{
    int prime[2] = {0, 0};
    bool tracked = false;
    DVO_TRY(read_term_log(rob.mlog.as<int>(), 3, rob.log_its, seq, rob.last.as<float>(), out, s, [](float s2) { return s2 != 0.0f; },
                          [&](int l, int it, const int* r) {
                              memcpy(&out->s2[l][it], &r[0], sizeof(float));
                              out->median_bin[l][it] = r[1];
                              out->count[l][it] = r[2];
                          },
                          {prime, rob.prime_mn.as<int>() + 2 * (size_t)seq, sizeof prime}, &tracked));
    if (tracked) { out->prime_bin = prime[0]; out->prime_count = prime[1]; }
    return DVO_OK;
}

int Tracker::last_robust_histogram(int seq, uint32_t* counts, hipStream_t s) const
{
    return read_back(counts, rob.hist_last.as<uint32_t>() + (size_t)seq * DVO_MEDIAN_BINS, sizeof(uint32_t) * DVO_MEDIAN_BINS, s);
}

int Tracker::begin_terms(hipStream_t s, const GivenOnce* once)
{
    if (rob.on) {
        RobustBeginArgs ra{};
        ra.table = rob.table.as<RobustEntry>(); ra.last_s2 = rob.last.as<float>();
        ra.given = (once || rob.mode == DVO_ROBUST_SCALE_GIVEN) ? 1 : 0;
        ra.scales = (!once && ra.given) ? rob.scales.src : nullptr;
        ra.s2_all = once ? once->s2 : 0.0f;
        ra.n_seq = n_seq; ra.kind = rob.kind; ra.param = rob.param;
        launch_robust_begin(ra, s);
        rob.tracked = true;
    }
    if (rob.median()) {
        MedianBeginArgs ma{};
        ma.hist = rob.hist.as<unsigned>(); ma.hist_last = rob.hist_last.as<unsigned>(); ma.prime_mn = rob.prime_mn.as<int>();
        ma.n_seq = n_seq;
        launch_median_begin(ma, s);
    }
    if (aff.on) {
        AffineBeginArgs ba{};
        ba.table = aff.table.as<AffineEntry>(); ba.last = aff.last.as<float>(); ba.prime_ab = aff.prime.as<float>();
        ba.rows = (!once && aff.mode == DVO_AFFINE_GIVEN) ? aff.rows.src : nullptr;
        ba.a_all = once ? once->a : 1.0f; ba.b_all = once ? once->b : 0.0f;
        ba.n_seq = n_seq;
        launch_affine_begin(ba, s);
        aff.tracked = true;
    }
    if (geo.on) {
        DVO_HIP(hipMemsetAsync(geo.last.p, 0, geo.last.bytes, s));
        geo.tracked = true;
    }
    if (lm.on) {
        LmBeginArgs la{};
        la.table = lm.table.as<dvo_lm_entry>(); la.last = lm.last.as<dvo_lm_record>();
        la.lambda0 = lm.cfg.lambda0; la.n_seq = n_seq;
        launch_lm_begin(la, s);
        lm.tracked = true;
    }
    return DVO_OK;
}

void Tracker::end_terms(hipStream_t s)
{
    rob.end_push(s);
    aff.end_push(s);
    geo.end_push(s);
    lm.end_push(s);
}

int Tracker::apply_step_control(const dvo_lm_config* c, hipStream_t s)
{
    const bool enable = c && c->mode != DVO_LM_OFF;
    if (enable && !lm.table.p) {
        lm.log_its = log_iterations();
        DVO_TRY(lm.table.alloc(sizeof(dvo_lm_entry) * (size_t)n_seq));
        DVO_TRY(lm.last.alloc(sizeof(dvo_lm_record) * (size_t)n_seq));
        DVO_TRY(lm.log.alloc(sizeof(int) * 2 * (size_t)lm.log_its * (size_t)g.levels * (size_t)n_seq));
        DVO_HIP(hipMemsetAsync(lm.table.p, 0, lm.table.bytes, s));
        DVO_HIP(hipMemsetAsync(lm.last.p, 0, lm.last.bytes, s));
        DVO_HIP(hipMemsetAsync(lm.log.p, 0, lm.log.bytes, s));
    }
    lm.on = enable;
    if (enable) lm.cfg = *c;
    return DVO_OK;
}

int Tracker::last_step_control(dvo_lm_record* rec, hipStream_t s) const { return read_back(rec, lm.last.p, sizeof(dvo_lm_record) * (size_t)n_seq, s); }

int Tracker::last_step_control_log(int seq, dvo_lm_log* out, hipStream_t s) const
{
    return read_term_log(lm.log.as<int>(), 2, lm.log_its, seq, lm.last.as<dvo_lm_record>(), out, s,
                         [](const dvo_lm_record& r) { return r.n_first != 0; },
                         [&](int l, int it, const int* r) {
                             memcpy(&out->lambda[l][it], &r[0], sizeof(float));
                             out->decision[l][it] = r[1];
                         });
}

LmSolve Tracker::lm_solve_args(size_t q0, bool log) const
{
    LmSolve m{};
    m.table = lm.table.as<dvo_lm_entry>() + q0;
    m.last = lm.last.as<dvo_lm_record>() + q0;
    m.log = log ? lm.log.as<int>() + 2 * q0 * (size_t)lm.log_its * g.levels : nullptr;
    m.levels = g.levels; m.log_its = lm.log_its;
    m.lambda_up = lm.cfg.lambda_up; m.lambda_down = lm.cfg.lambda_down; m.lambda_floor = lm.cfg.lambda_floor;
    m.lambda_max = lm.cfg.lambda_max; m.min_valid_fraction = lm.cfg.min_valid_fraction;
    return m;
}

int Tracker::apply_geometric(const dvo_geometric_config* c, hipStream_t s)
{
    const bool enable = c && c->mode != DVO_GEOMETRIC_OFF;
    if (enable && !geo.last.p) {
        geo.log_its = log_iterations();
        DVO_TRY(geo.last.alloc(sizeof(float) * 4 * (size_t)n_seq));
        DVO_TRY(geo.log.alloc(sizeof(float) * 2 * (size_t)geo.log_its * (size_t)g.levels * (size_t)n_seq));
        DVO_HIP(hipMemsetAsync(geo.last.p, 0, geo.last.bytes, s));
        DVO_HIP(hipMemsetAsync(geo.log.p, 0, geo.log.bytes, s));
    }
    geo.on = enable;
    if (enable) { geo.weight = c->weight; geo.max_diff = c->max_diff; }
    return DVO_OK;
}

int Tracker::last_geometric(dvo_geometric_record* rec, hipStream_t s) const
{
    std::vector<float> rows((size_t)4 * n_seq);
    DVO_TRY(read_back(rows.data(), geo.last.p, sizeof(float) * rows.size(), s));
    for (int q = 0; q < n_seq; q++) {
        rec[q].n_geo = (int)rows[4 * (size_t)q];
        rec[q].mean_sq = rows[4 * (size_t)q + 1];
    }
    return DVO_OK;
}

int Tracker::last_geometric_log(int seq, dvo_geometric_log* out, hipStream_t s) const
{
    using Last = std::array<float, 4>;   // (n_geo, mean_sq, tracked, 0)
    return read_term_log(geo.log.as<float>(), 2, geo.log_its, seq, geo.last.as<Last>(), out, s, [](const Last& r) { return r[2] != 0.0f; },
                         [&](int l, int it, const float* r) {
                             out->n_geo[l][it] = (int)r[0];
                             out->sum_sq[l][it] = r[1];
                         });
}

GeoGn Tracker::geo_gn_args(size_t q0, int level, const float* ref_z) const
{
    GeoGn z{};
    z.ref_z = ref_z + q0 * (size_t)g.w[level] * g.h[level];   // (gn_view's offset of these sequences)
    z.weight = geo.weight; z.max_diff = geo.max_diff;
    return z;
}

GeoSolve Tracker::geo_solve_args(size_t q0, bool log, double* sums_out) const
{
    GeoSolve z{};
    z.last = geo.last.as<float>() + 4 * q0;
    z.log = log ? geo.log.as<float>() + 2 * q0 * (size_t)geo.log_its * g.levels : nullptr;
    z.sums_out = sums_out;
    z.levels = g.levels; z.log_its = geo.log_its;
    return z;
}

int Tracker::apply_affine(const dvo_affine_config* c, hipStream_t s)
{
    const bool enable = c && c->mode != DVO_AFFINE_OFF;
    if (enable && !aff.table.p) {
        aff.log_its = log_iterations();
        DVO_TRY(aff.table.alloc(sizeof(AffineEntry) * (size_t)n_seq));
        DVO_TRY(aff.last.alloc(sizeof(float) * 2 * (size_t)n_seq));
        DVO_TRY(aff.prime.alloc(sizeof(float) * 2 * (size_t)n_seq));
        DVO_TRY(aff.rows.dev.alloc(sizeof(float) * 2 * (size_t)n_seq));
        DVO_TRY(aff.rows.stage.alloc(sizeof(float) * 2 * (size_t)n_seq));
        DVO_TRY(aff.moments.alloc(sizeof(float) * 8 * part_rows * (size_t)n_seq));
        DVO_TRY(aff.log.alloc(sizeof(float) * 2 * (size_t)aff.log_its * (size_t)g.levels * (size_t)n_seq));
        DVO_HIP(hipMemsetAsync(aff.last.p, 0, aff.last.bytes, s));
        DVO_HIP(hipMemsetAsync(aff.prime.p, 0, aff.prime.bytes, s));
        DVO_HIP(hipMemsetAsync(aff.log.p, 0, aff.log.bytes, s));
    }
    aff.on = enable;
    if (enable) {
        if (aff.mode != c->mode || c->mode != DVO_AFFINE_GIVEN) aff.rows.clear();   // (rows belong to one GIVEN configuration)
        aff.mode = c->mode; aff.min_pixels = c->min_pixels; aff.min_contrast = c->min_contrast;
        aff.gain_min = c->gain_min; aff.gain_max = c->gain_max;
    } else {
        aff.rows.clear();
        aff.mode = DVO_AFFINE_OFF;
    }
    return DVO_OK;
}

int Tracker::last_affine(float* ab, hipStream_t s) const { return read_back(ab, aff.last.p, sizeof(float) * 2 * (size_t)n_seq, s); }

int Tracker::last_affine_log(int seq, dvo_affine_log* out, hipStream_t s) const
{
    using Last = std::array<float, 2>;   // the last used (a, b)
    float prime[2] = {0.0f, 0.0f};
    bool tracked = false;
    DVO_TRY(read_term_log(aff.log.as<float>(), 2, aff.log_its, seq, aff.last.as<Last>(), out, s,
                          [](const Last& ab) { return !(ab[0] == 0.0f && ab[1] == 0.0f); },
                          [&](int l, int it, const float* r) {
                              out->a[l][it] = r[0];
                              out->b[l][it] = r[1];
                          },
                          {prime, aff.prime.as<float>() + 2 * (size_t)seq, sizeof prime}, &tracked));
    if (tracked) { out->prime_a = prime[0]; out->prime_b = prime[1]; }
    return DVO_OK;
}

AffineGn Tracker::affine_gn_args(size_t q0, bool prime) const
{
    AffineGn f{};
    f.table = aff.table.as<AffineEntry>() + q0;
    f.moments = aff.moments.as<float>() + q0 * part_rows * 8;
    f.prime = prime ? 1 : 0;
    return f;
}

AffineSolve Tracker::affine_solve_args(size_t q0, bool log, bool prime, double* moments_out, bool estimate_once) const
{
    AffineSolve f{};
    f.table = aff.table.as<AffineEntry>() + q0;
    f.moments = aff.moments.as<float>() + q0 * part_rows * 8;
    f.last = aff.last.as<float>() + 2 * q0;
    f.log = (log && !prime) ? aff.log.as<float>() + 2 * q0 * (size_t)aff.log_its * g.levels : nullptr;
    f.prime_ab = aff.prime.as<float>() + 2 * q0;
    f.moments_out = moments_out;
    f.levels = g.levels; f.log_its = aff.log_its;
    f.estimate = (aff.mode == DVO_AFFINE_ESTIMATE || estimate_once) ? 1 : 0;
    f.prime = prime ? 1 : 0;
    f.robust = rob.on ? 1 : 0;
    f.min_pixels = aff.min_pixels; f.min_contrast = aff.min_contrast; f.gain_min = aff.gain_min; f.gain_max = aff.gain_max;
    return f;
}

RobustSolve Tracker::robust_solve_args(size_t q0, bool adaptive) const
{
    RobustSolve r{};
    r.table = rob.table.as<RobustEntry>() + q0;
    r.last_s2 = rob.last.as<float>() + q0;
    r.kind = rob.kind; r.adaptive = adaptive ? 1 : 0;
    r.param = rob.param; r.floor2 = rob.floor2;
    return r;
}

MedianSolve Tracker::median_solve_args(size_t q0, bool log, bool prime, int* step_mn) const
{
    MedianSolve m{};
    m.hist = rob.hist.as<unsigned>() + q0 * DVO_MEDIAN_BINS;
    m.hist_last = rob.hist_last.as<unsigned>() + q0 * DVO_MEDIAN_BINS;
    m.log = (log && !prime) ? rob.mlog.as<int>() + 3 * q0 * (size_t)rob.log_its * g.levels : nullptr;
    m.prime_mn = rob.prime_mn.as<int>() + 2 * q0;
    m.step_mn = step_mn;
    m.levels = g.levels; m.log_its = rob.log_its;
    m.prime = prime ? 1 : 0;
    return m;
}

// false from the kernel file's tables: a set of terms without a kernel pair (Tracker::refusal lets none through), or `what`: a level
// planned as DVO_PLAN_ITERATION without a k_track_gn_fused instance (Tracker::init plans none)
static int term_launch_status(bool launched, const char* what = "no kernel pair for the opt-in terms that are on")
{
    if (launched) return DVO_OK;
    set_error(std::string("internal error: ") + what);
    return DVO_ERR_HIP;
}

int Tracker::launch_gn_term(const GnArgs& a, int level, int count, hipStream_t s, int grid_seqs, const float* ref_z, bool prime) const
{
    const LevelPlan& L = lv[level];
    const size_t q0 = (size_t)(a.state - state.as<SeqState>());
    TileTerms t{};
    t.on = terms_on();
    if (!t.on) { launch_gn(a, level, count, s, grid_seqs); return DVO_OK; }   // (the LDS-patch schedule is the plain plan's)
    if (rob.on) t.rob.table = rob.table.as<RobustEntry>() + q0;
    if (rob.median()) t.med.hist = rob.hist.as<unsigned>() + q0 * DVO_MEDIAN_BINS;
    if (aff.on) t.aff = affine_gn_args(q0, prime);
    if (geo.on) t.geo = geo_gn_args(q0, level, ref_z);
    return term_launch_status(launch_track_gn_terms(a, t, count, L.ppt, L.group, L.tiling.t2d != 0, s, grid_seqs));
}

int Tracker::launch_solve_term(const SolveArgs& sa, int count, hipStream_t s, const SolveTerm& st) const
{
    const size_t q0 = (size_t)(sa.state - state.as<SeqState>());
    const bool log = sa.log != nullptr;
    SolveTerms t{};
    t.on = terms_on();
    if (rob.on) t.rob = robust_solve_args(q0, st.adaptive_scale);
    if (rob.median()) t.med = median_solve_args(q0, log, st.prime, st.step_mn);
    if (aff.on) t.aff = affine_solve_args(q0, log, st.prime, st.affine_moments, st.estimate_once);
    if (geo.on) t.geo = geo_solve_args(q0, log, st.geo_sums);
    if (lm.on) t.lm = lm_solve_args(q0, log);
    return term_launch_status(launch_gn_solve_terms(sa, t, count, s));
}

void Tracker::launch_gn(const GnArgs& a, int level, int count, hipStream_t s, int grid_seqs) const
{
    const LevelPlan& L = lv[level];
    if (L.schedule == DVO_PLAN_LDS_PATCH) launch_track_gn_tile(a, count, L.ppt, s);
    else launch_track_gn(a, count, L.ppt, L.group, L.tiling.t2d != 0, s, grid_seqs);   // (the probe and the one-evaluation ops: any level)
}

GnArgs Tracker::gn_view(const GnArgs& all, int level, int q0, const TrackPlan* plan, const Intr* seq_k) const
{
    const size_t level_px = (size_t)g.w[level] * g.h[level];
    GnArgs ga = all;
    ga.obj_gray += q0 * level_px; ga.ref_gray += q0 * level_px; ga.ref_depth += q0 * level_px;
    if (ga.ref_wgt) ga.ref_wgt += q0 * level_px;
    ga.state += q0;
    // (a level-independent stride: with q0 * nblk[level], sub-batch k at a coarse level wrote into the rows of sub-batch k - 1
    //  at a finer level while both ran -- the nondeterminism of track_streams = 2 recorded in DESIGN.md section 12)
    ga.partials += (size_t)q0 * part_rows * 32;
    if (plan) ga.plan_action = plan->action + q0;
    if (seq_k) ga.seq_k = seq_k + (size_t)level * n_seq + q0;   // this level's row, this sub-batch
    return ga;
}

// One level of k_track_persist: the level's GnArgs, plus what GnArgs does not carry
static PersistLevel persist_level(const GnArgs& ga, const GnTiling& tl)
{
    PersistLevel L{};
    L.obj_gray = ga.obj_gray; L.ref_gray = ga.ref_gray; L.ref_depth = ga.ref_depth; L.ref_wgt = ga.ref_wgt; L.wgt_const = ga.wgt_const;
    L.inv_w = ga.inv_w; L.w = ga.w; L.h = ga.h; L.nblk = ga.nblk; L.q256 = ga.q256; L.r256 = ga.r256; L.k = ga.k; L.prm = ga.prm;
    L.blk_first = ga.blk_first; L.blk_count = ga.blk_count; L.t_shift = ga.t_shift; L.x_org = ga.x_org; L.y_org = ga.y_org;
    L.tiles_x = ga.tiles_x; L.t2d = tl.t2d; L.level_pixels = (int)tl.live_pixels;
    return L;
}

int Tracker::next_result_tag()
{
    result_tag = (result_tag + 1) & 0x1fffff;
    if (result_tag == 0) result_tag = 1;
    return result_tag;
}

int Tracker::track_persist(const FrameSet& obj, const FrameSet& ref, hipStream_t s)
{
    PersistArgs pa{};
    pa.levels = g.levels;
    for (int l = 0; l < g.levels; l++) pa.lv[l] = persist_level(gn_args(obj, ref, l, nullptr, 0), lv[l].tiling);
    pa.state = state.as<SeqState>(); pa.partials = partials.as<float>(); pa.log = log.as<dvo_track_log>();
    pa.ctl = persist_ctl.as<int>();
    pa.max_iterations = cfg.max_iterations; pa.fixed_iterations = cfg.fixed_iterations;
    pa.min_update = cfg.min_update; pa.min_residual = cfg.min_residual;
    pa.xi_out = xi_out.as<float>(); pa.T_out = T_out.as<float>(); pa.host_result = d_result;
    pa.host_tag = next_result_tag();
    pa.spin_limit = persist_spin_limit;
    pa.mono = mono_tail;
    if (persist_timeline) {   // diagnostic: stamps of the solver and of worker 0 (tools/persist_timeline.py reads them back)
        if (!persist_dbg.p) { DVO_TRY(persist_dbg.alloc(2 * 64 * 8 * sizeof(long long))); }
        DVO_HIP(hipMemsetAsync(persist_dbg.p, 0, persist_dbg.bytes, s));
        pa.dbg = persist_dbg.as<long long>();
        pa.dbg_worker = persist_dbg_worker;
    }
    if (!launch_track_persist(pa, lv[0].ppt, lv[0].group, persist_grid, s)) return DVO_OK;
    persist_used = true;
    DVO_HIP(hipGetLastError());
    return DVO_OK;
}

// The adaptive schedule's bounded wait for a word in mapped host memory that a kernel queued on `s` sets to a non-zero value
static int wait_progress(const volatile int* word, hipStream_t s)
{
    long spins = 0;
    while (*word == 0) {
        if (++spins > 2000000000L) {
            (void)hipStreamSynchronize(s);  // nothing may be left writing the progress words / state when we return
            set_error("adaptive schedule: the GPU made no progress");
            return DVO_ERR_HIP;
        }
        __builtin_ia32_pause();
    }
    return DVO_OK;
}

// One track() call's state, shared by the pieces of Tracker::track
struct TrackCall {
    hipStream_t s; const TrackPlan* plan;     // the caller's stream (sub-batch 0's) and plan
    const Intr* seq_k;                        // per-sequence intrinsics: the plan's table, or without a plan the per-camera mono batch's (nullptr: Geometry::k)
    int subs, n_levels, max_it;               // sub-batches (on s and sub_streams[0 .. subs - 2]), levels and iterations per level this call queues
    bool poll, top_waited;                    // the <= 8-sequence read-back paces this call; no stream has to wait for top_ready any more
    volatile int* prog_h; int* prog_d;        // adaptive: this call's progress words, host and device view
    int* rep_set;                             // k_track_gn_fused: this call's report words
    Tracker::SolveTerm iteration;             // every iteration's solve
};

static const char* const kLevelName[DVO_MAX_LEVELS] = {"track level 0", "track level 1", "track level 2", "track level 3", "track level 4",
                                                       "track level 5", "track level 6", "track level 7"};

// obj's top level: the split build's side stream writes it (every launch form reads it).  The first `streams` of the call wait, once.
int Tracker::wait_top(TrackCall& c, int streams)
{
    if (c.top_waited) return DVO_OK;
    for (int k = 0; k < streams; k++) DVO_HIP(hipStreamWaitEvent(k == 0 ? c.s : sub_streams[k - 1], top_ready, 0));
    c.top_waited = true;
    return DVO_OK;
}

int Tracker::track_prologue(TrackCall& c)
{
    hipStream_t s = c.s;
    if (!c.plan) launch_track_begin(state.as<SeqState>(), log.as<dvo_track_log>(), n_seq, g.levels, s);
    if (seed) {   // the start pose of every TRACK sequence (dvo_batch_set_pose_guess_mode), before the fork
        if (seed_mono) launch_mono_seed(*seed, s);
        else launch_seed_pose(*seed, s);
    }
    DVO_TRY(begin_terms(s));
    c.iteration.adaptive_scale = rob.on && rob.mode == DVO_ROBUST_SCALE_ADAPTIVE;
    c.max_it = cfg.fixed_iterations > 0 ? cfg.fixed_iterations : cfg.max_iterations;
    // Small batches: every few iterations ask the device whether anything is still active, so a converged
    // level does not pay for its remaining (empty) launches.  Big batches run the fixed schedule sync-free.
    c.poll = (cfg.fixed_iterations <= 0) && n_seq <= 8 && !adaptive;
    // (pinned: the read-back is one async copy + one stream sync, no staging)
    if (c.poll && !h_state) DVO_HIP(hipHostMalloc(reinterpret_cast<void**>(&h_state), sizeof(SeqState) * (size_t)n_seq, hipHostMallocDefault));
    // fork: the sub-batch streams start once everything queued on `s` so far (pyramids, k_track_begin) is done
    c.subs = c.poll ? 1 : n_sub;
    if (c.subs > 1) {
        DVO_HIP(hipEventRecord(ev_fork, s));
        for (int k = 1; k < c.subs; k++) DVO_HIP(hipStreamWaitEvent(sub_streams[k - 1], ev_fork, 0));
    }
    // adaptive: this call's progress words (the other set may still be written by the tail of the previous call)
    if (adaptive) {
        progress_set ^= 1;
        const size_t off = (size_t)progress_set * DVO_MAX_LEVELS * DVO_MAX_ITERATIONS;
        c.prog_h = h_progress + off; c.prog_d = d_progress + off;
        for (int i = 0; i < DVO_MAX_LEVELS * DVO_MAX_ITERATIONS; i++) c.prog_h[i] = 0;
    }
    bool any_iteration = false;
    for (int l = 0; l < g.levels; l++) any_iteration = any_iteration || lv[l].schedule == DVO_PLAN_ITERATION;
    c.rep_set = freport.as<int>() + (size_t)(progress_set & 1) * 2 * DVO_MAX_LEVELS * DVO_MAX_ITERATIONS;
    if (any_iteration) DVO_HIP(hipMemsetAsync(c.rep_set, 0, sizeof(int) * 2 * DVO_MAX_LEVELS * DVO_MAX_ITERATIONS, s));
    // adaptive schedule with a plan: k_plan's word says how many sequences track; with none, no level is launched at all
    c.n_levels = g.levels;
    if (adaptive && c.plan && c.plan->ready) {
        DVO_TRY(wait_progress(c.plan->ready, s));
        if (*c.plan->ready - 1 == 0) c.n_levels = 0;
    }
    return DVO_OK;
}

// Pacing ahead of iteration `it`, the adaptive schedule's: stay `ahead` iterations ahead of the GPU.  Wait until launch it-ahead of
// this level has reported: the caller stops the level if it had no active sequence -- every later launch of the level would be
// empty.  Skipping empty launches changes no result.  Two iterations ahead for every batch size: a batch iteration takes >= 20 us on
// the GPU, the host needs ~10 us to see a progress word and queue the next pair, and every iteration queued beyond the last useful
// one is an empty launch pair (~15 us): measured +1.6 % (mono, 1 iteration per level) / +0.7 % (sensor depth) against 4.
// Returns that word, the sequences that entered iteration it - ahead plus one (the active set only shrinks within a level, so they bound
// the list of `it`); 0: nothing to wait for; -1: the wait failed (the error is set).
int Tracker::wait_ahead(const TrackCall& c, int level, int it)
{
    const int ahead = 2;
    if (!adaptive || it < ahead) return 0;   // (k_track_level has no second iteration on the host)
    volatile int* pw = c.prog_h + level * DVO_MAX_ITERATIONS + (it - ahead);
    return wait_progress(pw, c.s) == DVO_OK ? *pw : -1;
}

// Pacing behind iteration `it`, a small batch's: ask the device whether anything is still active (*go = false: nothing is)
int Tracker::poll_active(const TrackCall& c, int level, int it, bool* go)
{
    if (!c.poll || lv[level].schedule == DVO_PLAN_LEVEL || it + 1 >= c.max_it) return DVO_OK;
    DVO_HIP(hipMemcpyAsync(h_state, state.p, sizeof(SeqState) * (size_t)n_seq, hipMemcpyDeviceToHost, c.s));
    DVO_HIP(hipStreamSynchronize(c.s));
    *go = false;
    for (int q = 0; q < n_seq; q++) *go = *go || h_state[q].active != 0;
    return DVO_OK;
}

// DVO_PLAN_LEVEL: the level iterates on the device, one k_track_level launch
void Tracker::queue_level(const GnArgs& ga, int level, int q0, int nq, hipStream_t sk)
{
    SolveArgs fa = solve_args(level, q0, 1, SolveRows::All);
    fa.partials = nullptr;
    launch_track_level(ga, fa, nq, sk);
}

// DVO_PLAN_ITERATION: GN accumulation + solve of this iteration in one launch (k_track_gn_fused).  init gives a level this schedule
// only where the launcher has an instance, so a refusal is an internal error.
int Tracker::queue_iteration(const TrackCall& c, const GnArgs& ga, int level, int it, int q0, int nq, hipStream_t sk)
{
    const LevelPlan& L = lv[level];
    const int word = level * DVO_MAX_ITERATIONS + it;
    const SolveArgs fa = solve_args(level, q0, it == 0, SolveRows::Live);
    return term_launch_status(launch_track_gn_fused(ga, fa, nq, L.ppt, L.group, L.tiling.t2d != 0, ticket.as<int>(), c.rep_set + 2 * word,
                                                    adaptive ? c.prog_d + word : nullptr, sk),
                              "no k_track_gn_fused instance for a level planned as DVO_PLAN_ITERATION");
}

// DVO_PLAN_PAIRS, DVO_PLAN_LDS_PATCH: one accumulation and one solve launch, through the opt-in terms that are on
//   ga: the sub-batch's view of the level (by value: the lists are filled in here); ref_z: the reference's depth of the level
int Tracker::queue_pair(const TrackCall& c, GnArgs ga, int level, int it, int k, int q0, int nq, hipStream_t sk, int active_ub, const float* ref_z)
{
    const bool lists = lv[level].schedule == DVO_PLAN_PAIRS;  // (k_track_gn_tile keeps the per-sequence active flag test)
    const SolveRows rows = pair_rows(level, SolveRows::LivePair);
    const int first = (it == 0) ? 1 : 0;
    // iteration `it` evaluates the sequences k_gn_solve(it - 1) left active (all of them when it == 0; with a plan the
    // plan's sequences of this sub-batch) and clears the list k_gn_solve(it) appends to
    const int* plan_list = c.plan ? c.plan->lists + (size_t)k * (size_t)(n_seq + 4) : nullptr;
    const int* list_prev = first ? plan_list : (lists ? work_list(k, it - 1) : nullptr);
    ga.list = list_prev;
    if (((aff.on && aff.mode == DVO_AFFINE_ESTIMATE) || rob.median()) && level == 0 && first) {
        // the priming pair: the moments (the median scale: the bin counts) of the start pose on the coarsest level give
        // the first iteration's entry; it leaves the pose, the log, the lists and the quality record alone
        DVO_TRY(launch_gn_term(ga, level, nq, sk, 0, ref_z, true));
        SolveArgs sp = solve_args(level, q0, 1, rows);
        sp.list_in = list_prev; sp.result = nullptr;
        SolveTerm tp{};
        tp.prime = true;
        DVO_TRY(launch_solve_term(sp, nq, sk, tp));
    }
    ga.next_count = lists ? work_list(k, it) : nullptr;
    if (cfg.profile) {
        if (ev_used == ev_pool.size()) {
            hipEvent_t e0, e1;
            DVO_HIP(hipEventCreate(&e0));
            DVO_HIP(hipEventCreate(&e1));
            ev_pool.emplace_back(e0, e1);
        }
        DVO_HIP(hipEventRecord(ev_pool[ev_used].first, sk));
    }
    DVO_TRY(launch_gn_term(ga, level, nq, sk, active_ub, ref_z));
    if (cfg.profile) DVO_HIP(hipEventRecord(ev_pool[ev_used++].second, sk));
    SolveArgs sa = solve_args(level, q0, first, rows);
    sa.counters = cfg.profile ? counters.as<unsigned long long>() : nullptr;   // (they describe k_track_gn launches only)
    sa.list_in = list_prev;
    sa.list_out = ga.next_count;
    if (adaptive) sa.progress = c.prog_d + level * DVO_MAX_ITERATIONS + it;
    return launch_solve_term(sa, nq, sk, c.iteration);
}

int Tracker::track(const FrameSet& obj, const FrameSet& ref, hipStream_t s, const TrackPlan* plan)
{
    TrackCall c{s, plan, plan ? plan->seq_k : cam_k};
    last_obj = &obj; last_ref = &ref;
    persist_used = false;
    c.top_waited = top_ready == nullptr;
    if (persist_call(plan)) {   // the whole call in one launch (k_track_persist)
        DVO_TRY(wait_top(c, 1));
        DVO_TRY(track_persist(obj, ref, s));
        if (persist_used) return DVO_OK;
    }
    DVO_TRY(track_prologue(c));
    for (int level = 0; level < c.n_levels; level++) {  // tracker.cpp:32
        TraceRange tr(kLevelName[level]);
        const int schedule = lv[level].schedule;
        const int host_its = schedule == DVO_PLAN_LEVEL ? 1 : c.max_it;  // (k_track_level iterates on the device)
        for (int it = 0; it < host_its; it++) {        // tracker.cpp:42
            const int first = (it == 0) ? 1 : 0;
            const int entered = wait_ahead(c, level, it);
            if (entered < 0) return DVO_ERR_HIP;
            if (entered == 1) break;
            const int active_ub = (entered && schedule != DVO_PLAN_ITERATION) ? entered - 1 : 0;
            if (level == g.levels - 1) DVO_TRY(wait_top(c, c.subs));   // before the top level's first launch, on every stream that launches it
            // (the geometric term: pixel x of the tracked frame uses that frame's own depth and weight; the reference's depth is sampled)
            const GnArgs ga0 = geo.on ? gn_args(obj.gray[level], ref.gray[level], obj.depth[level], obj.sigma_by_validity ? nullptr : obj.wgt[level],
                                                obj.sigma_by_validity ? obj.wgt_valid[level] : 0.0f, level, nullptr, first)
                                      : gn_args(obj, ref, level, nullptr, first);
            for (int k = 0; k < c.subs; k++) {  // launches of the sub-batches interleave on their streams
                const int q0 = c.subs > 1 ? sub_first(k) : 0, nq = (c.subs > 1 ? sub_first(k + 1) : n_seq) - q0;
                hipStream_t sk = k == 0 ? s : sub_streams[k - 1];
                const GnArgs ga = gn_view(ga0, level, q0, plan, c.seq_k);  // view of sequences [q0, q0 + nq)
                switch (schedule) {
                case DVO_PLAN_LEVEL: queue_level(ga, level, q0, nq, sk); break;
                case DVO_PLAN_ITERATION: DVO_TRY(queue_iteration(c, ga, level, it, q0, nq, sk)); break;
                case DVO_PLAN_PAIRS:
                case DVO_PLAN_LDS_PATCH: DVO_TRY(queue_pair(c, ga, level, it, k, q0, nq, sk, active_ub, ref.depth[level])); break;
                default: return term_launch_status(false, "a level without a schedule");
                }
            }
            bool go = true;
            DVO_TRY(poll_active(c, level, it, &go));
            if (!go) break;
        }
    }
    // join: `s` continues (pose export, the caller's next frame) only after every sub-batch chain has finished
    for (int k = 1; k < c.subs; k++) {
        DVO_HIP(hipEventRecord(ev_join[k - 1], sub_streams[k - 1]));
        DVO_HIP(hipStreamWaitEvent(s, ev_join[k - 1], 0));
    }
    DVO_TRY(wait_top(c, 1));   // (no level was launched: the caller's stream still orders obj's maps)
    if (h_result) next_result_tag();
    launch_export_poses(state.as<SeqState>(), xi_out.as<float>(), T_out.as<float>(), n_seq, s, d_result, result_tag);
    DVO_HIP(hipGetLastError());
    return DVO_OK;
}

int Tracker::read_persist_timeline(long long* out)   // [2][64][8]
{
    if (!persist_dbg.p) return DVO_ERR_NOT_READY;
    DVO_HIP(hipMemcpy(out, persist_dbg.p, persist_dbg.bytes, hipMemcpyDeviceToHost));
    return DVO_OK;
}

int Tracker::enable_host_result()
{
    if (h_result) return DVO_OK;
    DVO_HIP(hipHostMalloc(reinterpret_cast<void**>(&h_result), 64 * sizeof(float), hipHostMallocMapped | hipHostMallocCoherent));
    memset(h_result, 0, 64 * sizeof(float));
    DVO_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&d_result), h_result, 0));
    return DVO_OK;
}

int Tracker::wait_host_result(hipStream_t s, float xi[6], float T[16])
{
    if (!h_result) { set_error("host result not enabled"); return DVO_ERR_NOT_READY; }
    volatile int* tag = reinterpret_cast<volatile int*>(h_result + 22);
    volatile int* gave_up = reinterpret_cast<volatile int*>(h_result + 23);
    long spins = 0;
    while (*tag != result_tag) {
        __builtin_ia32_pause();
        if (persist_used && *gave_up == result_tag) {
            // k_track_persist ran into its polling limit (its workgroups were not all resident: the GPU is shared with something
            // that fills it).  Let it drain, reset its words and run this frame -- and every later one -- launch by launch.
            DVO_HIP(hipStreamSynchronize(s));
            DVO_HIP(hipMemset(persist_ctl.p, 0, persist_ctl.bytes));
            persist_failed = true;
            if (!last_obj || !last_ref) { set_error("k_track_persist gave up and the frame sets are gone"); return DVO_ERR_HIP; }
            DVO_TRY(track(*last_obj, *last_ref, s));
            spins = 0;
            continue;
        }
        if ((++spins & 0xfffff) == 0) {   // every ~1 M polls: has the stream finished (or failed) without the tag appearing?
            const hipError_t q = hipStreamQuery(s);
            if (q == hipSuccess) {
                if (*tag == result_tag) break;
                set_error("track(): the stream drained but the result tag never arrived");
                return DVO_ERR_HIP;
            }
            if (q != hipErrorNotReady) { set_error(hipGetErrorString(q)); return DVO_ERR_HIP; }
        }
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    for (int i = 0; i < 6; i++) xi[i] = h_result[i];
    for (int i = 0; i < 16; i++) T[i] = h_result[6 + i];
    return DVO_OK;
}

int Tracker::collect_profile(hipStream_t s)
{
    DVO_HIP(hipStreamSynchronize(s));
    for (size_t i = 0; i < ev_used; i++) {
        float ms = 0;
        DVO_HIP(hipEventElapsedTime(&ms, ev_pool[i].first, ev_pool[i].second));
        prof_ms += ms;
        prof_launches++;
    }
    ev_used = 0;
    return DVO_OK;
}

// ------------------------------------------------------------------------------------------------ keyframes
int Keyframe::alloc(const Geometry& g, const dvo_config& cfg, KeyframePool* from)
{
    const size_t top = sizeof(float) * (size_t)g.w[g.top()] * g.h[g.top()];
    if (from) {   // one block of the pool: [arena | age | depth_alt], each 256-byte aligned
        const size_t a0 = (FrameSet::arena_bytes(g, 1) + 255) & ~(size_t)255, a1 = (top + 255) & ~(size_t)255;
        void* blk = nullptr;
        DVO_TRY(from->take(a0 + 2 * a1, &blk));
        pool = from; block = blk;
        DVO_TRY(fs.alloc(g, 1, cfg, blk));
        age.adopt(static_cast<char*>(blk) + a0, top);
        depth_alt.adopt(static_cast<char*>(blk) + a0 + a1, top);
    } else {
        DVO_TRY(fs.alloc(g, 1, cfg));
        DVO_TRY(age.alloc(top));
        DVO_TRY(depth_alt.alloc(top));
    }
    depth_spare = depth_alt.as<float>();
    return DVO_OK;
}

// ------------------------------------------------------------------------------------------------ VisualOdometry
int VisualOdometry::fetch_valid_updates()
{
    if (!valid_updates_pending) return DVO_OK;
    DVO_TRY(select_device(device));
    DVO_HIP(hipMemcpyAsync(&last_valid_updates, valid_dev.p, sizeof(int), hipMemcpyDeviceToHost, stream));
    DVO_HIP(hipStreamSynchronize(stream));
    valid_updates_pending = false;
    return DVO_OK;
}

int VisualOdometry::fetch_log()
{
    if (!log_src) return DVO_OK;
    DVO_TRY(select_device(device));
    DVO_HIP(hipMemcpyAsync(&last_log, log_src->log.p, sizeof last_log, hipMemcpyDeviceToHost, stream));
    DVO_HIP(hipStreamSynchronize(stream));
    log_src = nullptr;
    return DVO_OK;
}

int VisualOdometry::upload_streams()
{
    if (ustream[0]) return DVO_OK;
    for (int i = 0; i < 2; i++) DVO_HIP(hipStreamCreateWithFlags(&ustream[i], hipStreamNonBlocking));
    for (int i = 0; i < 3; i++) DVO_HIP(hipEventCreateWithFlags(&uevent[i], hipEventDisableTiming));   // [2]: the mono frame's upload
    return DVO_OK;
}

VisualOdometry::~VisualOdometry()
{
    for (int i = 0; i < 2; i++) {
        if (ustream[i]) { (void)hipStreamSynchronize(ustream[i]); (void)hipStreamDestroy(ustream[i]); }
    }
    for (int i = 0; i < 3; i++)
        if (uevent[i]) (void)hipEventDestroy(uevent[i]);
    if (h_pin) (void)hipHostFree(h_pin);
    if (h_stage) { if (stream) (void)hipStreamSynchronize(stream); (void)hipHostFree(h_stage); }
    if (h_tables) { if (stream) (void)hipStreamSynchronize(stream); (void)hipHostFree(h_tables); }
    if (own_stream && stream) (void)hipStreamDestroy(stream);
}

int VisualOdometry::init(const float K9[9], int width, int height, const dvo_config* c)
{
    if (!K9 || width < 64 || height < 64) {
        set_error("dvo_vo_create: bad K or frame size");
        return DVO_ERR_BAD_ARGUMENT;
    }
    if (c) cfg = *c; else dvo_config_default(&cfg);
    memcpy(K, K9, sizeof K);
    w = width; h = height; device = cfg.device;
    DVO_TRY(select_device(device));
    if (cfg.stream) stream = (hipStream_t)cfg.stream;
    else { DVO_HIP(hipStreamCreate(&stream)); own_stream = true; }
    stage_mono_rows = getenv("DVO_MONO_STAGE") == nullptr || atoi(getenv("DVO_MONO_STAGE")) != 0;   // (read per handle: tests compare both paths)
    stage_raw_rows = getenv("DVO_RAW_STAGE") == nullptr || atoi(getenv("DVO_RAW_STAGE")) != 0;
    DVO_TRY(make_geometry(K, w, h, 3, 2, geoM));  // system.hpp:47
    DVO_TRY(make_geometry(K, w, h, 4, 1, geoD));  // system.hpp:82
    const size_t n = (size_t)w * h * sizeof(float);
    DVO_TRY(in_gray.alloc(n)); DVO_TRY(in_depth.alloc(n)); DVO_TRY(in_sigma.alloc(n));
    const size_t tn = (size_t)geoM.w[2] * geoM.h[2];
    DVO_TRY(tmp_a.alloc(tn * 4)); DVO_TRY(tmp_b.alloc(tn * 4)); DVO_TRY(tmp_c.alloc(tn * 4));
    DVO_TRY(owner.alloc(tn * 4));
    DVO_TRY(valid_dev.alloc(sizeof(int)));
    DVO_TRY(meta_dev.alloc(sizeof(MonoSeq)));
    DVO_HIP(hipMemset(meta_dev.p, 0, sizeof(MonoSeq)));
    DVO_HIP(hipHostMalloc(&h_pin, sizeof(MonoSeq) + sizeof(dvo_track_log), hipHostMallocDefault));  // pinned: the per-frame read-back is one DMA
    memset(&h_meta, 0, sizeof h_meta);
    memset(&last_log, 0, sizeof last_log);
    return DVO_OK;
}

void default_initial_depth(int n, uint32_t seed, std::vector<float>& d, std::vector<float>& s)
{  // stands in for cv::randn(depth, 1.5, 0.5); max(depth, 0.5); sigma = 0.5 (frame.hpp:17-21), deviation D6
    d.resize(n); s.assign(n, 0.5f);
    for (int i = 0; i < n; i++) {
        const uint32_t a = mix32(seed ^ (uint32_t)(2 * i + 1) * 0x9E3779B9U), b = mix32(a ^ 0x85EBCA6BU);
        const float u1 = ((float)(a >> 8) + 1.0f) * (1.0f / 16777217.0f), u2 = (float)(b >> 8) * (1.0f / 16777216.0f);
        const float z = std::sqrt(-2.0f * std::log(u1)) * std::cos(6.2831853f * u2);
        const float v = 1.5f + 0.5f * z;
        d[i] = v < 0.5f ? 0.5f : v;
    }
}

int VisualOdometry::set_distortion(const float D[5])
{
    if (fed) { set_error("dvo_vo_set_distortion: the handle has consumed a frame (D is fixed from the first frame on)"); return DVO_ERR_NOT_READY; }
    DVO_TRY(select_device(device));
    DVO_TRY(und.set("dvo_vo_set_distortion", D, false, 1, K, false, geoM, stream));
    return pho.rebuild(1, geoM, und, stream);   // (a calibration set before D: its gains move to the remap's source pixels)
}

int VisualOdometry::set_photometric(const float* resp, const float* vign)
{
    if (fed) { set_error("dvo_vo_set_photometric: the handle has consumed a frame (the calibration is fixed from the first frame on)"); return DVO_ERR_NOT_READY; }
    DVO_TRY(select_device(device));
    return pho.set("dvo_vo_set_photometric", (resp || vign) ? 1 : 0, resp, vign, nullptr, 1, geoM, und, stream);
}

// the sensor-depth entry points and init_keyframe have no defined meaning on a handle that undistorts or calibrates (include/dvo.h)
static int refuse_distorted(const VisualOdometry& vo, const char* who)
{
    if (vo.pho.enabled()) {
        set_error(std::string(who) + ": the handle has a photometric calibration (dvo_vo_set_photometric), which needs raw mono frames (dvo_vo_odometrize_raw)");
        return DVO_ERR_BAD_ARGUMENT;
    }
    if (!vo.und.enabled()) return DVO_OK;
    set_error(std::string(who) + ": the handle undistorts its frames (dvo_vo_set_distortion); sensor-depth input is not undistorted");
    return DVO_ERR_BAD_ARGUMENT;
}

int VisualOdometry::init_keyframe(const float* gray, const float* depth, const float* sigma)
{  // system.hpp:24-32 with the mono geometry (deviation D9)
    DVO_TRY(refuse_distorted(*this, "dvo_vo_init_keyframe"));
    if (!gray || !depth || !sigma) { set_error("null image"); return DVO_ERR_BAD_ARGUMENT; }
    fed = true;
    DVO_TRY(select_device(device));
    const size_t n = (size_t)w * h * sizeof(float);
    DVO_HIP(hipMemcpyAsync(in_gray.p, gray, n, hipMemcpyHostToDevice, stream));
    DVO_HIP(hipMemcpyAsync(in_depth.p, depth, n, hipMemcpyHostToDevice, stream));
    DVO_HIP(hipMemcpyAsync(in_sigma.p, sigma, n, hipMemcpyHostToDevice, stream));
    auto kf = std::make_unique<Keyframe>();
    DVO_TRY(kf->alloc(geoM, cfg, &kf_pool));
    kf->id = ++latest_id;
    build_pyramid(kf->fs, in_gray.as<float>(), in_depth.as<float>(), in_sigma.as<float>(), stream);
    DVO_HIP(hipMemsetAsync(kf->age.p, 0, kf->age.bytes, stream));
    DVO_HIP(hipStreamSynchronize(stream));
    hist.push_back(std::move(kf));
    hist_version++;
    return DVO_OK;
}

int VisualOdometry::map_propagate(Keyframe& frame, const Keyframe& ref)
{  // Mapper::propagate, mapper.cpp:62-74; the pose exp(+rel_xi) is the one k_mono_decide left in meta_dev
    const int T = geoM.top(), tw = geoM.w[T], th = geoM.h[T];
    PropArgs a{};
    a.ref_depth = ref.fs.depth[T]; a.ref_sigma = ref.fs.sigma[T]; a.ref_age = ref.age.as<float>();
    a.depth = frame.fs.depth[T]; a.sigma = frame.fs.sigma[T]; a.age = frame.age.as<float>();
    a.owner = owner.as<int>();
    a.w = tw; a.h = th; a.n_seq = 1; a.k = geoM.k[T];
    a.meta = meta_dev.as<MonoSeq>();
    launch_propagate_batch(a, stream);
    // (Frame::updateDepthSigmaAge, frame.cpp:47-54, re-decimates both maps here; Mapper::regularize and Frame::updateDepth follow at
    //  once, mapper.cpp:26, and decimate the depth again: map_regularize() derives every level of both pyramids in its one pass)
    return DVO_OK;
}

static const size_t kStageLimitBytes = 512 * 1024;

int VisualOdometry::alloc_stage()
{  // pinned, device-mapped: [colour / gray rows, up to 4 bytes per pixel][16-bit depth rows]
    if (h_stage) return DVO_OK;
    DVO_HIP(hipHostMalloc(&h_stage, (size_t)w * h * 6, hipHostMallocMapped));
    DVO_HIP(hipHostGetDevicePointer(&d_stage, h_stage, 0));
    return DVO_OK;
}

static void stage_rows_host(void* dst, const void* src, size_t row_bytes, int rows, int culls, bool decimate)
{  // the rows the pyramid keeps (every 2^culls-th) -- or all of them -- packed
    if (!decimate || culls <= 0) { memcpy(dst, src, row_bytes * (size_t)rows); return; }
    const int kept = rows >> culls;
    for (int r = 0; r < kept; r++)
        memcpy(static_cast<char*>(dst) + (size_t)r * row_bytes, static_cast<const char*>(src) + ((size_t)r << culls) * row_bytes, row_bytes);
}

int VisualOdometry::refresh_history_tables()
{  // device copies of FrameHistory's poses and top-level gray pointers (+ room for the age table): current after this call
    const int T = geoM.top();
    const int n_hist = (int)hist.size();
    if (hist_table_version == hist_version && hist_table_n == n_hist) return DVO_OK;
    // Staged in PINNED host memory, copied without a synchronisation: the staging block is rewritten only by a later call of this
    // function, i.e. in a later frame, and every frame waits for its tracking result, which is stream-ordered after these copies.
    const size_t xi_bytes = sizeof(float) * 6 * (size_t)n_hist, gt_bytes = sizeof(float*) * (size_t)n_hist;
    if (h_tables_bytes < xi_bytes + gt_bytes) {
        DVO_HIP(hipStreamSynchronize(stream));   // (the old tables / staging block may still be read by queued work)
        if (h_tables) DVO_HIP(hipHostFree(h_tables));
        h_tables = nullptr;
        h_tables_bytes = 2 * (xi_bytes + gt_bytes);
        DVO_HIP(hipHostMalloc(&h_tables, h_tables_bytes, hipHostMallocDefault));
        DVO_TRY(ages.alloc(sizeof(AgeEntry) * (size_t)n_hist * 2));
        DVO_TRY(hist_xi_dev.alloc(2 * xi_bytes));
        DVO_TRY(gray_tab_dev.alloc(2 * gt_bytes));
    }
    float* hx = static_cast<float*>(h_tables);
    const float** gt = reinterpret_cast<const float**>(static_cast<char*>(h_tables) + xi_bytes);   // (xi_bytes is a multiple of 8)
    for (int i = 0; i < n_hist; i++) {
        memcpy(hx + (size_t)i * 6, hist[i]->xi, 6 * sizeof(float));
        gt[i] = hist[i]->fs.gray[T];
    }
    DVO_HIP(hipMemcpyAsync(hist_xi_dev.p, hx, xi_bytes, hipMemcpyHostToDevice, stream));
    DVO_HIP(hipMemcpyAsync(gray_tab_dev.p, gt, gt_bytes, hipMemcpyHostToDevice, stream));
    hist_table_n = n_hist; hist_table_version = hist_version;
    return DVO_OK;
}

int VisualOdometry::map_update(Keyframe& obj)
{  // Mapper::update, mapper.cpp:76-137
    Keyframe& ref = *hist.back();
    const int T = geoM.top(), tw = geoM.w[T], th = geoM.h[T];
    const int n_hist = (int)hist.size();
    // mapper.cpp:107: r_xi = concatenate(obj.xi, -born.xi), once per keyframe, on the device (k_age_table).  The keyframes' poses and
    // top-level gray pointers only change when FrameHistory does (a keyframe pushed, dropped or loaded): the device copies are
    // refreshed then (hist_version), not on every frame -- two uploads and a stream synchronisation less per tracked frame.
    DVO_TRY(refresh_history_tables());
    AgeTableArgs ta{};
    ta.meta = meta_dev.as<MonoSeq>(); ta.hist_xi = hist_xi_dev.as<float>(); ta.ages = ages.as<AgeEntry>();
    ta.n_seq = 1; ta.R = n_hist; ta.n_hist = n_hist;
    ta.zero_word = valid_dev.as<int>();   // mapper.cpp:136's count of this update (read back when dvo_vo_last_valid_updates asks)
    if (!age_table_done) launch_age_table(ta, stream);   // (done: the tail of k_track_persist computed it, odometrize())
    age_table_done = false;
    UpdateArgs a{};
    a.ref_depth = ref.fs.depth[T]; a.ref_sigma = ref.fs.sigma[T]; a.ref_age = ref.age.as<float>();
    a.obj_gray = obj.fs.gray[T];
    a.ages = ages.as<AgeEntry>();
    a.gray_table = gray_tab_dev.as<const float*>();
    a.meta = meta_dev.as<MonoSeq>();
    a.n_seq = 1; a.R = n_hist; a.n_hist = n_hist; a.w = tw; a.h = th; a.crop = cfg.crop_enable; a.obj_id = obj.id;
    a.clamp_age = history_limit > 0 ? 1 : 0;
    a.seed = cfg.rng_seed;
    a.k = geoM.k[T];
    memcpy(a.K9, geoM.K9[T], sizeof a.K9);
    a.valid_updates = valid_dev.as<int>();
    launch_depth_update(a, stream);
    valid_updates_pending = true;
    // (mapper.cpp:135's Frame::updateDepthSigma: folded into map_regularize(), as in map_propagate())
    return DVO_OK;
}

int VisualOdometry::map_regularize(Keyframe& kf)
{  // Mapper::regularize (mapper.cpp:139-144) + Frame::updateDepth (frame.cpp:56-61), together with the re-decimation of sigma that the
   // preceding propagate / update left pending (frame.cpp:39-54): every level of depth and sigma is a decimation of the top maps, so one
   // pass (k_regularize_redecimate, the batched pipeline's kernel) leaves the values the reference's three re-decimations leave
    const int T = geoM.top();
    RegDecArgs ra{};
    ra.depth = kf.fs.depth[T]; ra.sigma = kf.fs.sigma[T];
    ra.depth_top_out = kf.depth_spare;
    for (int l = 0; l < geoM.levels; l++) {
        ra.w[l] = geoM.w[l]; ra.h[l] = geoM.h[l];
        ra.depth_lv[l] = kf.fs.depth[l]; ra.sigma_lv[l] = kf.fs.sigma[l]; ra.wgt[l] = kf.fs.wgt[l];
        ra.step[l] = kf.fs.step[l];
    }
    ra.levels = geoM.levels; ra.n_seq = 1; ra.sigma_min = kf.fs.sigma_min; ra.sigma_max = kf.fs.sigma_max;
    kf.fs.sigma_by_validity = false;
    launch_regularize_redecimate(ra, stream);
    std::swap(kf.fs.depth[T], kf.depth_spare);   // the top-level depth map alternates between the arena block and depth_alt
    return DVO_OK;
}

int VisualOdometry::odometrize(const float* gray, float T_world[16], int* is_key, const uint8_t* raw, int raw_channels)
{  // system.hpp:44-74; `raw` != nullptr: the frame arrives as u8 gray / RGB(A) and is converted while the pyramid is built
    if ((!gray && !raw) || !T_world) { set_error("null argument"); return DVO_ERR_BAD_ARGUMENT; }
    if (raw && raw_channels != 1 && raw_channels != 3 && raw_channels != 4) { set_error("bad channel count"); return DVO_ERR_BAD_ARGUMENT; }
    if (!raw && pho.enabled()) {
        set_error("dvo_vo_odometrize: the handle has a photometric calibration (dvo_vo_set_photometric), which needs the byte: feed raw frames (dvo_vo_odometrize_raw)");
        return DVO_ERR_BAD_ARGUMENT;
    }
    DVO_TRY(select_device(device));
    fed = true;
    if (!trkM_ready) {   // one launch per track() call (k_track_persist), as the sensor-depth tracker
        trkM.prefer_persist = true;
        if (const char* e = getenv("DVO_MONO_PERSIST")) trkM.prefer_persist = atoi(e) != 0;
        trkM.persist_ppt = -1;   // the tile size of the other schedules
        if (const char* e = getenv("DVO_MONO_PERSIST_PPT")) trkM.persist_ppt = atoi(e);
        DVO_TRY(trkM.init(geoM, 1, cfg));
        if (trkM.persist_ok) DVO_TRY(trkM.enable_host_result());
        trkM_ready = true;
    }
    // The frame goes up on a stream of its own: the previous call returned with its mapping kernels (update / propagate, regularize)
    // still queued on `stream`, and a copy queued behind them would wait for them although it touches nothing they do -- the staging
    // buffers were last read by the previous frame's pyramid, which that call waited for (the pose read-back).  The pyramid waits
    // for the copy (event), then everything is in stream order again.
    // (r3, later) ... or no copy at all: the mono pyramid keeps one row in four (cull 2), 77-307 KB of the frame.  The caller's thread
    // copies those rows into a pinned, device-mapped staging block -- what the runtime's own path for pageable memory starts with -- and
    // k_pyramid reads them from there over the host link; the runtime's copy (API + DMA + 22-37 us until the dependent kernel starts,
    // profiles/r03_mono_single_trace_final.txt) drops out.  The block was last read by the previous frame's pyramid, which that call waited
    // for.  DVO_MONO_STAGE=0: the copy on the side stream, as before.
    FrameInput fin;
    // only the rows the pyramid keeps are copied / cross PCIe -- whole frames when they are undistorted (the remap reads any row)
    fin.rows_decimated = decimate_host_rows && can_decimate_rows(geoM) && !und.enabled();
    const size_t row_bytes = raw ? (size_t)w * raw_channels : (size_t)w * sizeof(float);
    // (a thread's memcpy beats the runtime's copy path up to about half a megabyte -- measured at 77-460 KB; above that the DMA engine wins)
    const bool stage_rows = stage_mono_rows && row_bytes * (size_t)(fin.rows_decimated ? h >> geoM.culls : h) <= kStageLimitBytes;
    if (stage_rows) {
        if (!h_stage) {
            DVO_TRY(alloc_stage());
        }
        stage_rows_host(h_stage, raw ? static_cast<const void*>(raw) : static_cast<const void*>(gray), row_bytes, h, geoM.culls, fin.rows_decimated);
        if (raw) { fin.rgb = static_cast<const uint8_t*>(d_stage); fin.channels = raw_channels; }
        else fin.gray = static_cast<const float*>(d_stage);
    } else {
        DVO_TRY(upload_streams());
        hipStream_t up = ustream[1];
        if (raw) {
            const size_t px = (size_t)w * h;
            if (raw_rgb.bytes < px * 4) {
                DVO_HIP(hipStreamSynchronize(stream));
                DVO_TRY(raw_rgb.alloc(px * 4)); DVO_TRY(raw_depth.alloc(px * 2));
            }
            DVO_TRY(upload_rows(raw_rgb.p, raw, row_bytes, h, 1, geoM.culls, fin.rows_decimated, up, nullptr));
            fin.rgb = raw_rgb.as<uint8_t>(); fin.channels = raw_channels;
        } else {
            DVO_TRY(upload_rows(in_gray.p, gray, row_bytes, h, 1, geoM.culls, fin.rows_decimated, up, nullptr));
            fin.gray = in_gray.as<float>();
        }
        DVO_HIP(hipEventRecord(uevent[2], up));
        DVO_HIP(hipStreamWaitEvent(stream, uevent[2], 0));
    }
    if (!scratch) { scratch = std::make_unique<Keyframe>(); DVO_TRY(scratch->alloc(geoM, cfg, &kf_pool)); }
    Keyframe& frame = *scratch;
    frame.id = ++latest_id;
    for (int i = 0; i < 6; i++) { frame.xi[i] = 0; frame.rel_xi[i] = 0; }
    und.apply(fin, 1);   // dvo_vo_set_distortion: k_pyramid_remap
    pho.apply(fin, 1);   // dvo_vo_set_photometric: k_pyramid_raw4_photo / k_pyramid_photo
    build_pyramid(frame.fs, fin, stream);
    if (is_key) *is_key = 0;
    const int T = geoM.top();
    const size_t tn = (size_t)geoM.w[T] * geoM.h[T];
    if (hist.empty()) {  // system.hpp:49-54
        if (init_depth.empty()) default_initial_depth((int)tn, cfg.rng_seed, init_depth, init_sigma);
        DVO_HIP(hipMemcpyAsync(frame.fs.depth[T], init_depth.data(), tn * 4, hipMemcpyHostToDevice, stream));
        DVO_HIP(hipMemcpyAsync(frame.fs.sigma[T], init_sigma.data(), tn * 4, hipMemcpyHostToDevice, stream));
        DVO_HIP(hipMemsetAsync(frame.age.p, 0, frame.age.bytes, stream));
        redecimate(frame.fs, frame.fs.depth[T], frame.fs.sigma[T], stream);
        DVO_HIP(hipStreamSynchronize(stream));
        hist.push_back(std::move(scratch));
        hist_version++;
        const float z[6] = {0, 0, 0, 0, 0, 0};
        se3_exp_f(z, T_world);
        if (is_key) *is_key = 1;
        return DVO_OK;
    }
    Keyframe& ref = *hist.back();
    // Frame::updateXi (frame.cpp:7-14), Mapper::needNewFrame (mapper.cpp:45-60) and exp(xi) (system.hpp:73) on the device; the host keeps
    // FrameHistory, so the reference keyframe's pose and id go along as kernel arguments.  On the one-launch schedule they are the tail
    // of k_track_persist and everything the host needs arrives in the mapped block with the tracker's tag: no further launch, no copy,
    // no stream synchronisation.  Otherwise: k_mono_decide (the batched pipeline's kernel) + one copy.
    MonoRef hdr{};
    memcpy(hdr.ref_xi, ref.xi, sizeof hdr.ref_xi);
    hdr.ref_id = ref.id; hdr.n_total = (int)hist.size(); hdr.valid = 1;
    trkM.mono_tail = {};
    if (trkM.persist_call()) {
        PersistMono& pm = trkM.mono_tail;
        pm.meta = meta_dev.as<MonoSeq>();
        memcpy(pm.ref_xi, ref.xi, sizeof pm.ref_xi);
        pm.ref_id = ref.id; pm.n_total = (int)hist.size();
        pm.frame_id = frame.id; pm.max_frames = cfg.keyframe_max_frames; pm.min_translation = cfg.keyframe_min_translation;
        pm.enabled = 1;
        // ... and Mapper::update's per-keyframe relative poses (k_age_table), which only need the frame's pose and FrameHistory's
        DVO_TRY(refresh_history_tables());
        pm.hist_xi = hist_xi_dev.as<float>(); pm.ages = ages.as<AgeEntry>(); pm.n_hist = (int)hist.size();
        pm.zero_word = valid_dev.as<int>();
    }
    DVO_TRY(trkM.track(frame.fs, ref.fs, stream));  // system.hpp:57
    bool decided = false;
    if (trkM.persist_used) {
        float rel[6], Trel[16];
        DVO_TRY(trkM.wait_host_result(stream, rel, Trel));   // (a launch that gave up is re-run launch by launch in there: persist_used is false then)
        if (trkM.persist_used) {
            memcpy(h_meta.rel_xi, rel, sizeof h_meta.rel_xi);
            memcpy(h_meta.frame_xi, trkM.h_result + 24, sizeof h_meta.frame_xi);
            memcpy(h_meta.T_world, trkM.h_result + 30, sizeof h_meta.T_world);
            h_meta.need = reinterpret_cast<const int*>(trkM.h_result)[46];
            decided = true;
            age_table_done = h_meta.need == 0;   // (the same launch computed the age table for the update that follows)
        }
    }
    if (!decided) {
        launch_mono_decide(meta_dev.as<MonoSeq>(), trkM.state.as<SeqState>(), 1, frame.id, cfg.keyframe_min_translation, cfg.keyframe_max_frames,
                           nullptr, nullptr, nullptr, &hdr, stream);
        DVO_HIP(hipMemcpyAsync(h_pin, meta_dev.p, sizeof(MonoSeq), hipMemcpyDeviceToHost, stream));
        DVO_HIP(hipStreamSynchronize(stream));
        memcpy(&h_meta, h_pin, sizeof h_meta);
    }
    log_src = &trkM;   // (the 15 KB per-iteration log is read back when dvo_vo_last_track_log asks for it)
    memcpy(frame.rel_xi, h_meta.rel_xi, sizeof frame.rel_xi);
    memcpy(frame.xi, h_meta.frame_xi, sizeof frame.xi);
    frame.ref_id = ref.id;
    const bool need = h_meta.need != 0;
    memcpy(last_xi, frame.xi, sizeof last_xi);
    memcpy(last_rel, frame.rel_xi, sizeof last_rel);
    last_id = frame.id;
    memcpy(T_world, h_meta.T_world, 16 * sizeof(float));
    if (need) {
        DVO_TRY(map_propagate(frame, ref));
        hist.push_back(std::move(scratch));
        hist_version++;
        if (is_key) *is_key = 1;
        if (history_limit > 0 && (int)hist.size() > history_limit) {  // bounded store: drop the oldest keyframes
            DVO_HIP(hipStreamSynchronize(stream));                    // their buffers may still be read by queued kernels
            hist.erase(hist.begin(), hist.begin() + ((int)hist.size() - history_limit));
            hist_version++;
        }
    } else {
        DVO_TRY(map_update(frame));
    }
    DVO_TRY(map_regularize(*hist.back()));  // mapper.cpp:26,30
    DVO_HIP(hipGetLastError());
    return DVO_OK;
}

int VisualOdometry::odometrize_depth(const float* gray, const float* depth, const float* sigma, float T_rel[16])
{  // system.hpp:77-93
    DVO_TRY(refuse_distorted(*this, "dvo_vo_odometrize_depth"));
    if (!gray || !depth || !sigma || !T_rel) { set_error("null argument"); return DVO_ERR_BAD_ARGUMENT; }
    fed = true;
    DVO_TRY(select_device(device));
    if (!trkD_ready) { trkD.prefer_persist = true; DVO_TRY(trkD.init(geoD, 1, cfg)); trkD_ready = true; }
    FrameInput in;   // float maps: only the rows the pyramid keeps cross PCIe (upload_rows)
    in.rows_decimated = decimate_host_rows && can_decimate_rows(geoD);
    const size_t rb = (size_t)w * sizeof(float);
    // Tracking this frame needs its GRAY pyramid only (obj) -- depth, sigma and the weight come from the reference, the previous frame
    // (tracker.cpp:22-41).  So only the gray map's copy + pyramid sit on the critical path; the depth and sigma maps go up on a side
    // stream and their pyramid is built there WHILE this frame is tracked (three strided copies in a row were 98 us between one frame's
    // tracking and the next, profiles/r03_single_hip_trace.txt; one is ~30).  The next call makes the tracking stream wait for that
    // build (this frame is then the reference); this call returns only after the side copies have read the caller's buffers.
    DVO_TRY(upload_streams());
    if (!depth_cur) { depth_cur = std::make_unique<Keyframe>(); DVO_TRY(depth_cur->alloc(geoD, cfg)); }
    if (side_built) DVO_HIP(hipStreamWaitEvent(stream, uevent[1], 0));   // the reference's depth / sigma / weight pyramid (built during the previous call)
    DVO_TRY(upload_rows(in_gray.p, gray, rb, h, 1, geoD.culls, in.rows_decimated, stream, nullptr));
    Keyframe* const target = depth_cur.get();
    const bool dec = in.rows_decimated;
    const std::function<int()> side = [&]() -> int {   // queued after this frame's pyramid + tracking launches: those are the critical path
        DVO_TRY(upload_rows(in_depth.p, depth, rb, h, 1, geoD.culls, dec, ustream[0], nullptr));
        DVO_TRY(upload_rows(in_sigma.p, sigma, rb, h, 1, geoD.culls, dec, ustream[0], nullptr));
        DVO_HIP(hipEventRecord(uevent[0], ustream[0]));
        build_pyramid(target->fs, nullptr, in_depth.as<float>(), in_sigma.as<float>(), ustream[0], true, dec);
        DVO_HIP(hipEventRecord(uevent[1], ustream[0]));
        side_built = true;
        return DVO_OK;
    };
    in.gray = in_gray.as<float>(); in.depth = nullptr; in.sigma = nullptr;
    const int rc = odometrize_depth_staged(T_rel, &in, &side);
    if (side_built) DVO_HIP(hipEventSynchronize(uevent[0]));   // (long done: the copies take ~50 us, the tracking ~270)
    return rc;
}

int VisualOdometry::odometrize_depth_raw(const uint8_t* rgb, int channels, const uint16_t* depth16, float depth_scale, float T_rel[16])
{  // the same call fed with raw sensor frames: u8 gray/RGB(A) + u16 depth, converted on the device while the pyramid is built
    DVO_TRY(refuse_distorted(*this, "dvo_vo_odometrize_depth_raw"));
    if (!rgb || !depth16 || !T_rel || (channels != 1 && channels != 3 && channels != 4)) { set_error("bad raw frame"); return DVO_ERR_BAD_ARGUMENT; }
    fed = true;
    DVO_TRY(select_device(device));
    const size_t px = (size_t)w * h;
    if (raw_rgb.bytes < px * 4) { DVO_TRY(raw_rgb.alloc(px * 4)); DVO_TRY(raw_depth.alloc(px * 2)); }
    FrameInput in;
    in.rows_decimated = decimate_host_rows && can_decimate_rows(geoD);   // only the rows the pyramid keeps cross PCIe
    DVO_TRY(upload_streams());
    if (side_built) { DVO_HIP(hipStreamWaitEvent(stream, uevent[1], 0)); side_built = false; }   // a float-map frame's depth pyramid may still be building: it is this call's reference
    // The kept rows of both frames (0.46 MB of 0.92 at cull 1) are staged by the caller's thread in pinned, device-mapped memory and read
    // from there by k_pyramid_raw4 -- no runtime copy (as in the mono loop; DVO_RAW_STAGE=0: two copies, the depth on the side stream).
    if (stage_raw_rows && ((size_t)w * channels + (size_t)w * 2) * (size_t)(in.rows_decimated ? h >> geoD.culls : h) <= kStageLimitBytes) {
        DVO_TRY(alloc_stage());
        char* hs = static_cast<char*>(h_stage);
        stage_rows_host(hs, rgb, (size_t)w * channels, h, geoD.culls, in.rows_decimated);
        stage_rows_host(hs + (size_t)w * h * 4, depth16, (size_t)w * 2, h, geoD.culls, in.rows_decimated);
        in.rgb = static_cast<const uint8_t*>(d_stage); in.channels = channels;
        in.depth16 = reinterpret_cast<const uint16_t*>(static_cast<const char*>(d_stage) + (size_t)w * h * 4); in.depth_scale = depth_scale;
        return odometrize_depth_staged(T_rel, &in);
    }
    DVO_TRY(upload_rows(raw_depth.p, depth16, (size_t)w * 2, h, 1, geoD.culls, in.rows_decimated, ustream[0], nullptr));
    DVO_HIP(hipEventRecord(uevent[0], ustream[0]));
    DVO_TRY(upload_rows(raw_rgb.p, rgb, (size_t)w * channels, h, 1, geoD.culls, in.rows_decimated, stream, nullptr));
    DVO_HIP(hipStreamWaitEvent(stream, uevent[0], 0));
    in.rgb = raw_rgb.as<uint8_t>(); in.channels = channels; in.depth16 = raw_depth.as<uint16_t>(); in.depth_scale = depth_scale;
    return odometrize_depth_staged(T_rel, &in);
}

int VisualOdometry::odometrize_depth_staged(float T_rel[16], const FrameInput* raw, const std::function<int()>* after_launch)
{
    if (!trkD_ready) { trkD.prefer_persist = true; DVO_TRY(trkD.init(geoD, 1, cfg)); trkD_ready = true; }
    if (!depth_cur) { depth_cur = std::make_unique<Keyframe>(); DVO_TRY(depth_cur->alloc(geoD, cfg)); }
    Keyframe& frame = *depth_cur;
    frame.id = ++latest_id;
    if (raw) build_pyramid(frame.fs, *raw, stream);   // (raw sensor frame or float maps staged by the caller)
    else build_pyramid(frame.fs, in_gray.as<float>(), in_depth.as<float>(), in_sigma.as<float>(), stream);
    const float z[6] = {0, 0, 0, 0, 0, 0};
    if (!depth_ref) {  // system.hpp:83-86
        for (int i = 0; i < 6; i++) { frame.xi[i] = 0; frame.rel_xi[i] = 0; }
        if (after_launch) DVO_TRY((*after_launch)());
        DVO_HIP(hipStreamSynchronize(stream));
        depth_ref = std::move(depth_cur);
        se3_exp_f(z, T_rel);
        return DVO_OK;
    }
    DVO_TRY(trkD.enable_host_result());
    DVO_TRY(trkD.track(frame.fs, depth_ref->fs, stream));
    if (after_launch) DVO_TRY((*after_launch)());   // (work that is not on this frame's critical path is queued once the tracking is)
    // The pose comes back through mapped host memory (k_export_poses' last store), not through a copy + stream synchronisation; the
    // caller's input buffers were consumed by copies that are stream-ordered before the kernels whose result this waits for.
    float rel[6];
    DVO_TRY(trkD.wait_host_result(stream, rel, T_rel));
    log_src = &trkD;   // the per-iteration log stays on the device until dvo_vo_last_track_log asks for it
    memcpy(frame.rel_xi, rel, sizeof rel);
    frame.ref_id = depth_ref->id;
    se3_concatenate_f(depth_ref->xi, rel, frame.xi);
    memcpy(last_xi, frame.xi, sizeof last_xi);
    memcpy(last_rel, rel, sizeof last_rel);
    last_id = frame.id;
    std::swap(depth_ref, depth_cur);  // m_ref_frame = frame, system.hpp:91
    return DVO_OK;
}

// ------------------------------------------------------------------------------------------------ batch
Batch::~Batch()
{
    if (pstream) { (void)hipStreamSynchronize(pstream); (void)hipStreamDestroy(pstream); }
    host.release();
    if (ev_last_track) (void)hipEventDestroy(ev_last_track);
    for (int i = 0; i < 3; i++) if (ev_built[i]) (void)hipEventDestroy(ev_built[i]);
    if (split.fork) (void)hipEventDestroy(split.fork);
    if (split.done) (void)hipEventDestroy(split.done);
    plan.release(stream);   // (host staging goes before the stream does: PinnedPair)
    cam_stage.release(stream);
    guess.release(stream);
    trk.rob.release(stream);
    trk.aff.release(stream);
    if (own_stream && stream) (void)hipStreamDestroy(stream);
}

int Batch::init(int n, const float K9[9], int w, int h, int levels, int culls, const dvo_config* c)
{
    if (n < 1 || !K9) { set_error("dvo_batch_create: bad arguments"); return DVO_ERR_BAD_ARGUMENT; }
    if (c) cfg = *c; else dvo_config_default(&cfg);
    n_seq = n; device = cfg.device;
    DVO_TRY(select_device(device));
    if (cfg.stream) stream = (hipStream_t)cfg.stream;
    else { DVO_HIP(hipStreamCreate(&stream)); own_stream = true; }
    DVO_TRY(make_geometry(K9, w, h, levels, culls, g));
    memcpy(K_create, K9, sizeof K_create);
    cam_K.resize((size_t)n * 9);
    for (int q = 0; q < n; q++) memcpy(&cam_K[(size_t)q * 9], K9, 9 * sizeof(float));
    cam_K_used = cam_K;
    for (int i = 0; i < 3; i++) DVO_TRY(fs[i].alloc(g, n, cfg));
    DVO_TRY(trk.init(g, n, cfg));
    {   // lowest priority: the pyramid build should fill what the tracker leaves idle, not compete with it
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        DVO_HIP(hipStreamCreateWithPriority(&pstream, hipStreamNonBlocking, lo));
    }
    DVO_HIP(hipEventCreateWithFlags(&ev_last_track, hipEventDisableTiming));
    for (int i = 0; i < 3; i++) DVO_HIP(hipEventCreateWithFlags(&ev_built[i], hipEventDisableTiming));
    {
        const char* e = getenv("DVO_PYRAMID_SPLIT");
        split_on = (e && e[0]) ? e[0] != '0' : n >= 1024;
        split.side = pstream;
        DVO_HIP(hipEventCreateWithFlags(&split.fork, hipEventDisableTiming));
        DVO_HIP(hipEventCreateWithFlags(&split.done, hipEventDisableTiming));
    }
    return DVO_OK;
}

// Builds the pyramids of a frame that will be handed to push_device later (call order per step: prefetch(k+1); push(k)) on the
// side stream.  The set it builds into may be the reference of the tracking queued last: the build waits for that tracking --
// not for anything queued afterwards -- and then runs beside the tracking of frame k.
// One frame of every sequence from HOST memory: up to three buffers (float gray / depth / sigma, or raw rgb / depth16) go to the
// staging slot of this push on the copy stream; the tracking stream waits for that copy only.  Slot k & 1 is reused by push k + 2,
// whose copy waits until push k (pyramid build + tracking) is done with it.
int Batch::check_actions_input(const FrameInput& in) const
{
    if (plan.act_pending && cur >= 0 && weights_by_validity(fs[cur], in) != fs[cur].sigma_by_validity) {   // (a SKIP copies the weight storage)
        set_error("dvo_batch_set_actions: a push with actions must keep the weight storage of the references (raw frames vs float maps)");
        return DVO_ERR_BAD_ARGUMENT;
    }
    if (kf_on && cur >= 0 && weights_by_validity(fs[cur], in) != fs[cur].sigma_by_validity) {   // (a promotion copies the weight storage)
        set_error("dvo_batch_set_keyframe_tracking: every push must keep the weight storage of the keyframes (raw frames vs float maps)");
        return DVO_ERR_BAD_ARGUMENT;
    }
    return DVO_OK;
}

int Batch::push_host_frame(const void* p0, const void* p1, const void* p2, FrameInput in)
{
    DVO_TRY(check_actions_input(in));   // (before the copies are queued)
    DVO_TRY(select_device(device));
    // The adaptive schedule keeps the host inside track() until the GPU is nearly done with the frame; a host-fed batch wants the
    // next frame's transfer queued meanwhile, so it runs the fixed schedule (bit-identical results, tested).
    trk.adaptive = false;
    DVO_TRY(host.begin());
    // Known difference from MonoBatch::odometrize_host, kept: the frame counts as taken before its copies are queued, and the slot is
    // marked consumed below whatever push() returns (the mono batch stages a refused frame's successor into the same slot).
    host.advance();
    in.rows_decimated = host.decimate(g, und) && pyr_filter == DVO_PYRAMID_FILTER_NONE;   // (the filter reads every source row)
    const size_t rb = (size_t)g.src_w * (in.raw() ? (size_t)in.channels : sizeof(float));
    DVO_TRY(host.upload(0, p0, rb, g, n_seq, in.rows_decimated));
    if (p1) DVO_TRY(host.upload(1, p1, in.raw() ? (size_t)g.src_w * 2 : rb, g, n_seq, in.rows_decimated));
    if (p2) DVO_TRY(host.upload(2, p2, rb, g, n_seq, in.rows_decimated));
    DVO_TRY(host.end_copy(stream, host_buffer_is_pinned(p0) && (!p1 || host_buffer_is_pinned(p1)) && (!p2 || host_buffer_is_pinned(p2))));
    const HostStage::Slot& st = host.cur();
    if (in.raw()) { in.rgb = st.buf[0].as<uint8_t>(); in.depth16 = st.buf[1].as<uint16_t>(); }
    else { in.gray = st.buf[0].as<float>(); in.depth = st.buf[1].as<float>(); in.sigma = st.buf[2].as<float>(); }
    const int rc = push(in);
    DVO_TRY(host.consumed(stream));
    return rc;
}

// ------------------------------------------------------------------------------------------------ host-frame staging
int HostStage::begin()
{
    if (!cstream) {
        DVO_HIP(hipStreamCreateWithFlags(&cstream, hipStreamNonBlocking));
        for (auto& st : slot) {
            DVO_HIP(hipEventCreateWithFlags(&st.copied, hipEventDisableTiming));
            DVO_HIP(hipEventCreateWithFlags(&st.consumed, hipEventDisableTiming));
        }
    }
    k = n_push & 1;
    if (cur().used) DVO_HIP(hipStreamWaitEvent(cstream, cur().consumed, 0));
    return DVO_OK;
}

int HostStage::upload(int i, const void* src, size_t row_bytes, const Geometry& g, int n_seq, bool decimate)
{
    DevBuf& b = cur().buf[i];
    const size_t whole = row_bytes * (size_t)g.src_h * (size_t)n_seq;
    if (b.bytes < whole) DVO_TRY(b.alloc(whole));
    return upload_rows(b.p, src, row_bytes, g.src_h, (size_t)n_seq, g.culls, decimate, cstream, nullptr);
}

int HostStage::end_copy(hipStream_t tracking, bool all_sources_pinned)
{
    DVO_HIP(hipEventRecord(cur().copied, cstream));
    // Pageable memory: the runtime may pin it in place and return while the DMA is still reading it, and the caller is free to
    // release the buffer as soon as this call returns -- so wait for the copy (only the copy: the tracking of the previous frame
    // keeps running on the tracking stream).  Pinned buffers stay asynchronous, as the header says.
    if (!all_sources_pinned) DVO_HIP(hipStreamSynchronize(cstream));
    DVO_HIP(hipStreamWaitEvent(tracking, cur().copied, 0));
    return DVO_OK;
}

int HostStage::consumed(hipStream_t tracking)
{
    DVO_HIP(hipEventRecord(cur().consumed, tracking));
    cur().used = true;
    return DVO_OK;
}

void HostStage::release()
{
    if (cstream) { (void)hipStreamSynchronize(cstream); (void)hipStreamDestroy(cstream); cstream = nullptr; }
    for (auto& st : slot) {
        if (st.copied) { (void)hipEventDestroy(st.copied); st.copied = nullptr; }
        if (st.consumed) { (void)hipEventDestroy(st.consumed); st.consumed = nullptr; }
    }
}

int Batch::prefetch(const FrameInput& in)
{
    if (!in.key0() || !in.has_depth()) { set_error("null device pointer"); return DVO_ERR_BAD_ARGUMENT; }
    if (plan.act_pending) { set_error("dvo_batch_prefetch: actions are pending for the next push (prefetch and actions do not combine)"); return DVO_ERR_NOT_READY; }
    if (kf_on) { set_error("dvo_batch_prefetch: keyframe tracking is on (prefetch and keyframe tracking do not combine)"); return DVO_ERR_NOT_READY; }
    DVO_TRY(select_device(device));
    const int slot = free_slot();
    if (npre >= 2 || slot < 0) { set_error("dvo_batch_prefetch_device: two prefetched frames are already waiting for their push"); return DVO_ERR_NOT_READY; }
    FrameInput fin = in;
    fin.filter = pyr_filter;
    und.apply(fin, n_seq);   // dvo_batch_set_sensor_distortion: k_pyramid_remap_depth (device frames: whole)
    if (tracked_once) DVO_HIP(hipStreamWaitEvent(pstream, ev_last_track, 0));
    build_pyramid(fs[slot], fin, pstream, /*keep_sigma=*/false);
    DVO_HIP(hipEventRecord(ev_built[slot], pstream));
    preq[npre] = slot;
    pre_key[npre][0] = in.key0(); pre_key[npre][1] = in.key1();
    npre++;
    DVO_HIP(hipGetLastError());
    return DVO_OK;
}

int Batch::push(const FrameInput& in)
{
    if (!in.key0() || !in.has_depth()) { set_error("null device pointer"); return DVO_ERR_BAD_ARGUMENT; }
    DVO_TRY(select_device(device));
    // per-sequence path: actions pending, or used by an earlier push (then every push is an all-TRACK plan), or per-sequence intrinsics,
    // or keyframe tracking
    const bool planned = plan.act_pending || plan.act_used || cam_used || kf_on;
    DVO_TRY(check_actions_input(in));
    if (und.enabled() && in.rows_decimated) { set_error("internal: an undistorted frame needs whole frames"); return DVO_ERR_BAD_ARGUMENT; }
    if (pyr_filter && in.rows_decimated) { set_error("internal: a filtered pyramid needs whole frames"); return DVO_ERR_BAD_ARGUMENT; }
    FrameInput fin = in;
    fin.filter = pyr_filter;
    und.apply(fin, n_seq);   // dvo_batch_set_sensor_distortion: k_pyramid_remap_depth
    int target;
    bool built = false;
    if (npre > 0 && pre_key[0][0] == in.key0() && pre_key[0][1] == in.key1()) {
        target = preq[0];                                   // built by prefetch: the tracker waits for that build
        DVO_HIP(hipStreamWaitEvent(stream, ev_built[target], 0));
        preq[0] = preq[1];
        for (int i = 0; i < 2; i++) pre_key[0][i] = pre_key[1][i];
        npre--;
        built = true;
    } else {
        target = (cur < 0 && npre == 0) ? 0 : free_slot();
        if (target < 0) { set_error("dvo_batch_push_device: the frames prefetched must be pushed first, in order"); return DVO_ERR_BAD_ARGUMENT; }
    }
    PoseSeedArgs sa{};
    if (!planned) {
        // Frame(gray,depth,sigma,K,levels,culls); a big batch's raw frames: split, the top level and the depth maps on the side stream
        // (the geometric term reads the tracked frame's depth at every level: no split build while it is on)
        const bool halves = !built && build_pyramid(fs[target], fin, stream, /*keep_sigma=*/false, nullptr, nullptr,
                                                    (split_on && !trk.geo.on) ? &split : nullptr);
        DVO_HIP(split.err);
        if (cur >= 0) {
            if (guess.on()) { sa = guess.args(trk.state.as<SeqState>(), nullptr, DVO_SEQ_TRACK, trk.xi_out.as<float>(), nullptr); trk.seed = &sa; }
            trk.top_ready = halves ? split.done : nullptr;
            const int rc = trk.track(fs[target], fs[cur], stream);    // system.hpp:88
            trk.seed = nullptr; trk.top_ready = nullptr;
            if (rc != DVO_OK && halves) (void)hipStreamWaitEvent(stream, split.done, 0);   // (a failed call may not have queued the wait)
            DVO_TRY(rc);
            DVO_HIP(hipEventRecord(ev_last_track, stream));
            tracked_once = true;
            have_poses = true;
        } else {
            if (halves) DVO_HIP(hipStreamWaitEvent(stream, split.done, 0));   // (nothing tracks: the set is complete when the push is)
            seed_untracked(nullptr, DVO_SEQ_RESTART);
        }
    } else {
        // k_plan first (it reads only the actions and has_ref), then the pyramid: SKIP sequences copy their reference forward, so the
        // whole new frame set becomes the reference below (cur = target) and k_track_gn addresses frame sets as it always does
        const bool skips = plan.act_pending;   // (without pending actions every sequence builds: a prefetched set needs nothing more)
        DVO_TRY(launch_plan(cur >= 0));
        if (!built) build_pyramid(fs[target], fin, stream, /*keep_sigma=*/false, skips ? plan.eff.as<uint8_t>() : nullptr, cur >= 0 ? &fs[cur] : &fs[target]);
        if (cur >= 0) {
            TrackPlan tp = plan.track_plan(trk);
            tp.seq_k = cam_table();
            if (guess.on()) { sa = guess_args(plan.eff.as<uint8_t>(), 0); trk.seed = &sa; }
            const int rc = trk.track(fs[target], fs[cur], stream, &tp);
            trk.seed = nullptr;
            DVO_TRY(rc);
            DVO_HIP(hipEventRecord(ev_last_track, stream));
            tracked_once = true;
        } else {   // no frame set to track against yet: every sequence starts (or stays without a reference); k_plan zeroed the twists
            seed_untracked(plan.eff.as<uint8_t>(), 0);
            launch_export_poses(trk.state.as<SeqState>(), trk.xi_out.as<float>(), trk.T_out.as<float>(), n_seq, stream);
        }
        if (kf_on) DVO_TRY(update_keyframes(target));
        have_poses = true;
        plan.consumed();
        if (cam_pending) { cam_K_used = cam_K; cam_pending = false; }   // (k_plan has read this push's camera-changed bytes)
    }
    if (und_pending) { und_D_used = und.D; und_pending = false; }   // (the D this push used: the camera-change rule's reference)
    guess.given.clear();   // (rows are spent by the push that follows them)
    quality.ready = quality.on;
    trk.end_terms(stream);
    n_push++;
    if (!kf_on || cur < 0) {
        prev = cur;
        cur = target;                                       // system.hpp:91
    } else {                                                // keyframe tracking: the first push's set stays the keyframe set
        prev = target;                                      // (the last frame's set: dvo_batch_probe_gn's obj)
    }
    DVO_HIP(hipGetLastError());
    return DVO_OK;
}

// ------------------------------------------------------------------------------------------------ two-slot pinned staging
int PinnedPair::alloc(size_t bytes)
{
    for (int i = 0; i < 2; i++) {
        if (!h[i]) DVO_HIP(hipHostMalloc(&h[i], bytes, hipHostMallocDefault));
        if (!ev[i]) DVO_HIP(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
    }
    return DVO_OK;
}

int PinnedPair::acquire(void** host)
{
    const int k = slot;
    slot ^= 1;
    if (staged[k]) DVO_HIP(hipEventSynchronize(ev[k]));   // (that copy was queued two calls ago)
    *host = h[k];
    return DVO_OK;
}

int PinnedPair::commit(void* dst_dev, size_t bytes, hipStream_t s)
{
    const int k = slot ^ 1;   // (the block acquire() handed out last)
    DVO_HIP(hipMemcpyAsync(dst_dev, h[k], bytes, hipMemcpyHostToDevice, s));
    DVO_HIP(hipEventRecord(ev[k], s));
    staged[k] = true;
    return DVO_OK;
}

void PinnedPair::release(hipStream_t s)
{
    if (h[0] && s) (void)hipStreamSynchronize(s);
    for (int i = 0; i < 2; i++) {
        if (h[i]) { (void)hipEventSynchronize(ev[i]); (void)hipHostFree(h[i]); h[i] = nullptr; }
        if (ev[i]) { (void)hipEventDestroy(ev[i]); ev[i] = nullptr; }
        staged[i] = false;
    }
}

// ------------------------------------------------------------------------------------------------ per-sequence actions (both batch kinds)
int SeqPlan::alloc(int n_seq, int n_sub, bool has_ref_fill, hipStream_t s)
{
    if (has_ref.p) return DVO_OK;
    const size_t n = (size_t)n_seq;
    DVO_TRY(act_dev.alloc(n));
    DVO_TRY(eff.alloc((n + 3) & ~(size_t)3));   // (read as 32-bit words by the mono batch's k_regularize_redecimate_plan)
    DVO_TRY(status.alloc(sizeof(int) * n));
    DVO_TRY(lists.alloc(2 * sizeof(int) * (size_t)n_sub * (n + 4)));
    DVO_TRY(tally.alloc(2 * sizeof(int)));
    DVO_TRY(act_stage.alloc(n));
    if (!h_ready) {
        DVO_HIP(hipHostMalloc(reinterpret_cast<void**>(&h_ready), 2 * sizeof(int), hipHostMallocMapped | hipHostMallocCoherent));
        h_ready[0] = h_ready[1] = 0;
        DVO_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&d_ready), h_ready, 0));
    }
    DVO_TRY(has_ref.alloc(n));   // (last: alloc runs again until everything before it is there)
    // in stream order: after plain pushes / calls every sequence has a reference / keyframe; the list counts start at zero
    DVO_HIP(hipMemsetAsync(has_ref.p, has_ref_fill ? 1 : 0, n, s));
    DVO_HIP(hipMemsetAsync(lists.p, 0, lists.bytes, s));
    DVO_HIP(hipMemsetAsync(tally.p, 0, tally.bytes, s));
    return DVO_OK;
}

int SeqPlan::set_actions(const uint8_t* actions, bool on_device, int n_seq, hipStream_t s)
{
    if (!actions) { act_pending = false; act_src = nullptr; return DVO_OK; }
    if (on_device) {
        act_src = actions;   // read by k_plan in stream order
    } else {
        // copied now into pinned staging, then to the device in stream order (after the k_plan of every earlier push / call)
        void* h = nullptr;
        DVO_TRY(act_stage.acquire(&h));
        memcpy(h, actions, (size_t)n_seq);
        DVO_TRY(act_stage.commit(act_dev.p, (size_t)n_seq, s));
        act_src = act_dev.as<uint8_t>();
    }
    act_pending = true;
    return DVO_OK;
}

PlanArgs SeqPlan::plan_args(const Tracker& trk, bool track_follows)
{
    PlanArgs a{};
    a.actions = act_pending ? act_src : nullptr;
    a.has_ref = has_ref.as<uint8_t>(); a.eff = eff.as<uint8_t>(); a.status = status.as<int>();
    a.state = trk.state.as<SeqState>(); a.log = trk.log.as<dvo_track_log>(); a.levels = trk.g.levels;
    a.lists = list_set(trk, parity);
    a.lists_clear = list_set(trk, parity ^ 1);
    a.list_stride = trk.n_seq + 4; a.n_sub = trk.n_sub; a.n_seq = trk.n_seq;
    if (trk.adaptive && track_follows) {   // Tracker::track waits for this word (the one of this parity was last used two plans ago)
        h_ready[parity] = 0;
        a.ready = d_ready + parity;
        a.tally = tally.as<int>();
    }
    return a;
}

TrackPlan SeqPlan::track_plan(const Tracker& trk) const
{
    TrackPlan tp;
    tp.action = eff.as<uint8_t>();
    tp.lists = list_set(trk, parity);
    tp.ready = trk.adaptive ? h_ready + parity : nullptr;
    return tp;
}

// The push / call has queued everything that reads this plan.  act_src is nulled for both kinds: it is read only while act_pending
// is set, and set_actions always writes it before it sets act_pending.
void SeqPlan::consumed()
{
    act_pending = false; act_src = nullptr; act_used = true;
    parity ^= 1;
}

int SeqPlan::status_of_last(int* out, bool out_on_device, int n_seq, bool first_push, hipStream_t s) const
{
    if (!act_used) {   // plain pushes / calls: the first one starts every sequence, every later one tracks every sequence
        const int v = first_push ? DVO_SEQ_STARTED : DVO_SEQ_TRACKED;
        if (out_on_device) { DVO_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(out), v, (size_t)n_seq, s)); return DVO_OK; }
        DVO_HIP(hipStreamSynchronize(s));   // (as a read-back of the device buffer would)
        for (int q = 0; q < n_seq; q++) out[q] = v;
        return DVO_OK;
    }
    DVO_HIP(hipMemcpyAsync(out, status.p, sizeof(int) * (size_t)n_seq, out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    if (!out_on_device) DVO_HIP(hipStreamSynchronize(s));
    return DVO_OK;
}

void SeqPlan::release(hipStream_t s)
{
    act_stage.release(s);   // (drains s: the ready words, allocated only after the staging, are no longer written either)
    if (h_ready) { (void)hipHostFree(h_ready); h_ready = d_ready = nullptr; }
}

// ------------------------------------------------------------------------------------------------ batch: per-sequence actions
int Batch::set_actions(const uint8_t* actions, bool on_device)
{
    if (npre > 0) { set_error("dvo_batch_set_actions: a prefetched frame is waiting for its push (prefetch and actions do not combine)"); return DVO_ERR_NOT_READY; }
    if (actions) {
        DVO_TRY(select_device(device));
        DVO_TRY(alloc_plan());
    }
    return plan.set_actions(actions, on_device, n_seq, stream);
}

int Batch::launch_plan(bool track_follows)
{
    DVO_TRY(alloc_plan());
    PlanArgs a = plan.plan_args(trk, track_follows);
    a.cam_changed = cam_pending ? cam_changed() : nullptr;
    dvo::launch_plan(a, stream);
    DVO_HIP(hipGetLastError());
    return DVO_OK;
}

int Batch::status_of_last(int* out, bool out_on_device)
{
    if (n_push == 0) { set_error("dvo_batch_last_status: nothing has been pushed yet"); return DVO_ERR_NOT_READY; }
    DVO_TRY(select_device(device));
    return plan.status_of_last(out, out_on_device, n_seq, n_push == 1, stream);
}

// ------------------------------------------------------------------------------------------------ batch: per-sequence intrinsics
int Batch::set_intrinsics(const float* K)
{
    if (npre > 0) { set_error("dvo_batch_set_intrinsics: a prefetched frame is waiting for its push"); return DVO_ERR_NOT_READY; }
    const size_t n = (size_t)n_seq;
    if (K) DVO_TRY(check_intrinsics("dvo_batch_set_intrinsics", K, n));
    DVO_TRY(select_device(device));
    if (und.enabled()) {   // the undistortion camera of a sequence is its current K: new tables where fx, fy, cx or cy change
        std::vector<float> Kn(n * 9);
        bool moved = false;
        for (size_t q = 0; q < n; q++) {
            memcpy(&Kn[q * 9], K ? K + q * 9 : K_create, 9 * sizeof(float));
            for (int j : {0, 4, 2, 5}) moved = moved || memcmp(&Kn[q * 9 + j], &cam_K[q * 9 + j], sizeof(float)) != 0;
        }
        if (moved) {
            const std::vector<float> D = und.D;
            DVO_HIP(hipStreamSynchronize(stream));   // no queued push or (consumed) prefetch still reads the tables it replaces
            DVO_TRY(und.set("dvo_batch_set_intrinsics", D.data(), true, n_seq, Kn.data(), true, g, stream));
        }
    }
    return stage_cameras(K);
}

// the intrinsics table of the next push (pinned staging, then one copy in stream order) and its camera-changed bytes; the batch runs
// the per-sequence path from then on
int Batch::stage_cameras(const float* K)
{
    const size_t n = (size_t)n_seq;
    const size_t table = sizeof(Intr) * (size_t)g.levels * n, bytes = table + n;
    if (!cam_dev.p) DVO_TRY(cam_dev.alloc(bytes));
    DVO_TRY(cam_stage.alloc(bytes));
    // pinned staging (the copy of two calls ago has been read by then), filled in place, then one copy in stream order: every push
    // queued before this call has finished reading the device table when it is overwritten, and the next push reads the new one
    void* h = nullptr;
    DVO_TRY(cam_stage.acquire(&h));
    Intr* tab = static_cast<Intr*>(h);
    uint8_t* changed = static_cast<uint8_t*>(h) + table;
    for (size_t q = 0; q < n; q++) {
        const float* kq = K ? K + q * 9 : K_create;
        Intr lv[DVO_MAX_LEVELS];
        level_intrinsics(kq, g, lv);
        for (int l = 0; l < g.levels; l++) tab[(size_t)l * n + q] = lv[l];
        // camera-change rule: fx, fy, cx or cy differ in bits from the table of the last push, or D does (or goes between none and a row)
        const float* ku = &cam_K_used[q * 9];
        changed[q] = (memcmp(&kq[0], &ku[0], 4) | memcmp(&kq[4], &ku[4], 4) | memcmp(&kq[2], &ku[2], 4) | memcmp(&kq[5], &ku[5], 4)) != 0 ||
                     distortion_changed(q);
        if (kq != &cam_K[q * 9]) memcpy(&cam_K[q * 9], kq, 9 * sizeof(float));
    }
    DVO_TRY(cam_stage.commit(cam_dev.p, bytes, stream));
    cam_pending = true;
    cam_used = true;
    return DVO_OK;
}

// ------------------------------------------------------------------------------------------------ batch: lens undistortion
int Batch::set_pyramid_filter(int filter)
{
    if (filter != DVO_PYRAMID_FILTER_NONE && filter != DVO_PYRAMID_FILTER_BINOMIAL3) {
        set_error("dvo_batch_set_pyramid_filter: filter is not DVO_PYRAMID_FILTER_NONE or DVO_PYRAMID_FILTER_BINOMIAL3");
        return DVO_ERR_BAD_ARGUMENT;
    }
    if ((n_push > 0 || npre > 0) && filter != pyr_filter) {
        set_error("dvo_batch_set_pyramid_filter: the filter is fixed once the batch has seen a frame");
        return DVO_ERR_BAD_ARGUMENT;
    }
    if (filter != DVO_PYRAMID_FILTER_NONE && und.enabled()) {
        set_error("dvo_batch_set_pyramid_filter: the batch undistorts its frames (the filter and dvo_batch_set_sensor_distortion do not combine)");
        return DVO_ERR_BAD_ARGUMENT;
    }
    if (filter != DVO_PYRAMID_FILTER_NONE && g.culls > 2) {
        set_error("dvo_batch_set_pyramid_filter: the filtered build supports culls 0, 1 and 2");
        return DVO_ERR_BAD_ARGUMENT;
    }
    pyr_filter = filter;
    return DVO_OK;
}

int Batch::set_sensor_distortion(const float* D, bool per_sequence)
{
    if (pyr_filter != DVO_PYRAMID_FILTER_NONE) {
        set_error("dvo_batch_set_sensor_distortion: the batch filters its gray pyramid (dvo_batch_set_pyramid_filter does not combine with it)");
        return DVO_ERR_BAD_ARGUMENT;
    }
    if (npre > 0) { set_error("dvo_batch_set_sensor_distortion: a prefetched frame is waiting for its push"); return DVO_ERR_NOT_READY; }
    DVO_TRY(select_device(device));
    // Synchronous: the tables are replaced only once no queued push or (consumed) prefetch can still read them
    DVO_HIP(hipStreamSynchronize(stream));
    DVO_TRY(und.set("dvo_batch_set_sensor_distortion", D, per_sequence, n_seq, cam_K.data(), true, g, stream));
    und_pending = true;
    // before the first push nothing has a reference: the batch stays on the plain path.  After it, the change of camera goes to k_plan
    // through the camera-changed bytes, on the per-sequence path, as dvo_batch_set_intrinsics
    if (n_push > 0) return stage_cameras(cam_K.data());
    return DVO_OK;
}

// ------------------------------------------------------------------------------------------------ batch: start pose of the tracking
int PoseGuess::set_mode(int m, int n, hipStream_t s, const uint8_t* prev_eff_dev, int prev_all)
{
    if (!dev.p) {   // first mode set: rows, starts and history; the history starts from the push before (prev_eff_dev / prev_all)
        n_seq = n;
        DVO_TRY(dev.alloc(sizeof(float) * 24 * (size_t)n + 2 * (size_t)n));
        DVO_HIP(hipMemsetAsync(dev.p, 0, dev.bytes, s));
        if (prev_eff_dev) DVO_HIP(hipMemcpyAsync(prev_eff(), prev_eff_dev, (size_t)n, hipMemcpyDeviceToDevice, s));
        else DVO_HIP(hipMemsetAsync(prev_eff(), prev_all, (size_t)n, s));
        given.dev.adopt(rows(), sizeof(float) * 6 * (size_t)n);
        DVO_TRY(given.stage.alloc(sizeof(float) * 6 * (size_t)n));
    }
    mode = m;
    if (m != DVO_GUESS_GIVEN) given.clear();
    return DVO_OK;
}

PoseSeedArgs PoseGuess::args(SeqState* state, const uint8_t* eff, int all_eff, const float* last_xi, const MonoSeq* meta) const
{
    PoseSeedArgs a{};
    a.state = state; a.eff = eff; a.all_eff = all_eff; a.mode = mode;
    a.rows = mode == DVO_GUESS_GIVEN ? given.src : nullptr;
    a.start = start(); a.prev_eff = prev_eff(); a.last_xi = last_xi; a.hist = hist(); a.hist_n = hist_n(); a.meta = meta;
    a.n_seq = n_seq;
    return a;
}

int PoseGuess::last_start(float* out, hipStream_t s) const
{
    return read_back(out, start(), sizeof(float) * 6 * (size_t)n_seq, s);
}

int Batch::set_guess_mode(int m)
{
    DVO_TRY(select_device(device));
    // the push before: its effective actions (per-sequence path), else all STARTED (first push) or all TRACKED (later ones)
    const uint8_t* pe = plan.act_used ? plan.eff.as<uint8_t>() : nullptr;
    const int all = n_push == 0 ? 0xff : (n_push == 1 ? DVO_SEQ_RESTART : DVO_SEQ_TRACK);
    return guess.set_mode(m, n_seq, stream, pe, all);
}

PoseSeedArgs Batch::guess_args(const uint8_t* eff_dev, int all_eff)
{
    if (kf_on) return guess.args(trk.state.as<SeqState>(), eff_dev, all_eff, xi_world.as<float>(), kf_meta.as<MonoSeq>());
    return guess.args(trk.state.as<SeqState>(), eff_dev, all_eff, trk.xi_out.as<float>(), nullptr);
}

void Batch::seed_untracked(const uint8_t* eff_dev, int all_eff)
{
    if (!guess.on()) return;
    const PoseSeedArgs sa = guess_args(eff_dev, all_eff);
    if (kf_on) launch_mono_seed(sa, stream);
    else launch_seed_pose(sa, stream);
}

// ------------------------------------------------------------------------------------------------ batch: keyframe tracking
int Batch::set_keyframe_tracking(int enable)
{
    if (n_push > 0) { set_error("dvo_batch_set_keyframe_tracking: the tracking mode is chosen before the first push"); return DVO_ERR_NOT_READY; }
    if (enable && npre > 0) {
        set_error("dvo_batch_set_keyframe_tracking: a prefetched frame is waiting for its push (prefetch and keyframe tracking do not combine)");
        return DVO_ERR_NOT_READY;
    }
    if (enable && !kf_meta.p) {
        DVO_TRY(select_device(device));
        const size_t n = (size_t)n_seq;
        DVO_TRY(kf_meta.alloc(sizeof(MonoSeq) * n));
        DVO_TRY(xi_world.alloc(sizeof(float) * 6 * n));
        DVO_TRY(T_world.alloc(sizeof(float) * 16 * n));
        DVO_TRY(is_key.alloc(sizeof(int) * n));
        DVO_TRY(need_list.alloc(sizeof(int) * (n + 4)));
        DVO_HIP(hipMemsetAsync(kf_meta.p, 0, kf_meta.bytes, stream));   // n_total = 0: no sequence has started
    }
    kf_on = enable != 0;
    trk.seed_mono = kf_on;   // (a start pose is a world twist, as in a mono batch: k_mono_seed over kf_meta)
    return DVO_OK;
}

// After the tracking of a push: the keyframe rule of every TRACK sequence and the starts (k_kf_decide), then the frames of the sequences it
// listed -- gray, depth and (where the set stores them) wgt of every level -- over their keyframes in fs[cur] (k_promote: no ring, only
// the listed sequences; at most DVO_PROMOTE_MAX_SEG maps per launch).  SKIP sequences are not listed: their keyframes are not written.
int Batch::update_keyframes(int frame_set)
{
    const int kf = cur >= 0 ? cur : frame_set;   // (the first push: its set becomes the keyframe set, nothing to copy)
    DVO_HIP(hipMemsetAsync(need_list.p, 0, 4 * sizeof(int), stream));
    MonoPlanArgs ma{};
    ma.meta = kf_meta.as<MonoSeq>(); ma.state = trk.state.as<SeqState>(); ma.eff = plan.eff.as<uint8_t>();
    ma.xi_world = xi_world.as<float>(); ma.T_world = T_world.as<float>(); ma.is_key = is_key.as<int>(); ma.need_list = need_list.as<int>();
    ma.n_seq = n_seq; ma.R = 1; ma.max_frames = cfg.keyframe_max_frames; ma.min_translation = cfg.keyframe_min_translation;
    launch_kf_decide(ma, stream);
    const bool carried = carry_keyframes(frame_set, kf);   // (before the copy: the old keyframe is still there to gather from)
    if (frame_set == kf) return fuse_keyframes(frame_set, kf);   // (the first push: every sequence starts or stays empty)
    const FrameSet& src = fs[frame_set];
    FrameSet& dst = fs[kf];
    const float* from[3 * DVO_MAX_LEVELS];
    float* to[3 * DVO_MAX_LEVELS];
    int count[3 * DVO_MAX_LEVELS];
    int n = 0;
    for (int m = 0; m < 3; m++) {
        if (m == 2 && dst.sigma_by_validity) break;   // (raw frames with constant weights: no wgt maps)
        for (int l = 0; l < g.levels; l++, n++) {
            from[n] = m == 0 ? src.gray[l] : m == 1 ? src.depth[l] : src.wgt[l];
            to[n] = m == 0 ? dst.gray[l] : m == 1 ? dst.depth[l] : dst.wgt[l];
            count[n] = g.w[l] * g.h[l];
        }
    }
    for (int first = 0; first < n; first += DVO_PROMOTE_MAX_SEG) {
        PromoteArgs pa{};
        pa.n_seg = n - first < DVO_PROMOTE_MAX_SEG ? n - first : DVO_PROMOTE_MAX_SEG;
        for (int k = 0; k < pa.n_seg; k++) { pa.src[k] = from[first + k]; pa.dst[k] = to[first + k]; pa.count[k] = count[first + k]; }
        pa.n_seq = n_seq; pa.npix = 0; pa.R = 1;
        pa.meta = kf_meta.as<MonoSeq>(); pa.all = 0; pa.need_list = need_list.as<int>();
        launch_promote(pa, stream);
    }
    DVO_TRY(fuse_keyframes(frame_set, kf));
    if (carried) commit_carry();   // (k_kf_fuse has cleared the promoted sequences' counts)
    return DVO_OK;
}

// ------------------------------------------------------------------------------------------------ batch: keyframe depth fusion and carry
int Batch::KfStage::alloc(DevBuf& plane, size_t n_seq, size_t npix)
{
    if (plane.p) return DVO_OK;
    DVO_TRY(plane.alloc(n_seq * npix));
    DVO_TRY(table.alloc(sizeof(KfSeq) * n_seq));
    DVO_TRY(rec.alloc(sizeof(KfRecord) * n_seq));
    return DVO_OK;
}

KfPrepArgs Batch::kf_prep_args(const KfStage& st) const
{
    KfPrepArgs pa{};
    pa.meta = kf_meta.as<MonoSeq>(); pa.eff = plan.eff.as<uint8_t>(); pa.is_key = is_key.as<int>();
    pa.table = st.table.as<KfSeq>(); pa.rec = st.rec.as<KfRecord>(); pa.n_seq = n_seq;
    return pa;
}

template <class Args>
void Batch::kf_pixel_args(Args& a, const KfStage& st, float max_diff) const
{
    const int T = g.top();
    for (int l = 0; l < g.levels; l++) { a.w[l] = g.w[l]; a.h[l] = g.h[l]; }
    a.table = st.table.as<KfSeq>(); a.rec = st.rec.as<KfRecord>();
    a.seq_k = cam_table() ? cam_table() + (size_t)T * n_seq : nullptr;
    a.k = g.k[T];
    a.levels = g.levels; a.n_seq = n_seq;
    a.min_depth = cfg.min_depth; a.max_diff = max_diff; a.max_count = fuse.cfg.max_count;
}

int Batch::set_keyframe_fusion(const dvo_kf_fusion_config* c)
{
    const bool enable = c && c->mode == DVO_KF_FUSION_ON;
    if (enable && !fuse.on) {   // off -> on: the counts (re)start at 0
        DVO_TRY(select_device(device));
        const size_t n = (size_t)n_seq, npix = (size_t)g.w[g.top()] * g.h[g.top()];
        DVO_TRY(fuse.alloc(fuse.counts, n, npix));
        DVO_HIP(hipMemsetAsync(fuse.counts.p, 0, n * npix, stream));
    }
    if (enable) fuse.cfg = *c;
    fuse.on = enable;
    if (!enable) carry.on = false;   // (the carry needs the count plane kept up to date)
    return DVO_OK;
}

// After k_kf_decide and the promotions: k_kf_fuse_prep resolves every sequence to clear / fuse / nothing from what k_kf_decide left,
// k_kf_fuse works on the top level of fs[kf] in place and gathers from fs[frame_set] (on the first push the two are one set, and no
// sequence can fuse: none had a keyframe to track against).
int Batch::fuse_keyframes(int frame_set, int kf)
{
    fuse.ready = fuse.on;
    if (!fuse.on) return DVO_OK;
    fuse.ran = true;
    launch_kf_fuse_prep(kf_prep_args(fuse), stream);
    KfFuseArgs a{};
    kf_pixel_args(a, fuse, fuse.cfg.max_diff);
    for (int l = 0; l < g.levels; l++) a.kf_depth[l] = fs[kf].depth[l];
    a.frame_depth = fs[frame_set].depth[g.top()];
    a.counts = fuse.counts.as<uint8_t>();
    launch_kf_fuse(a, stream);
    return DVO_OK;
}

int Batch::set_keyframe_carry(const dvo_kf_carry_config* c)
{
    const bool enable = c && c->mode == DVO_KF_CARRY_ON;
    if (enable) {
        DVO_TRY(select_device(device));
        DVO_TRY(carry.alloc(carry.staged, (size_t)n_seq, (size_t)g.w[g.top()] * g.h[g.top()]));
        carry.cfg = *c;
    }
    carry.on = enable;
    return DVO_OK;
}

// After k_kf_decide and before the promotions: k_kf_carry_prep resolves every sequence to carry / nothing, k_kf_carry works on the depth
// pyramid of fs[frame_set] in place and gathers depth and counts from fs[kf] and the count plane, which nothing writes before k_promote
// and k_kf_fuse (on the first push the two sets are one and no sequence can carry: only the records are zeroed).
bool Batch::carry_keyframes(int frame_set, int kf)
{
    carry.ready = carry.on;
    if (!carry.on) return false;
    launch_kf_carry_prep(kf_prep_args(carry), stream);
    if (frame_set == kf) return false;
    KfCarryArgs a{};
    kf_pixel_args(a, carry, carry.cfg.max_diff);
    for (int l = 0; l < g.levels; l++) a.frame_depth[l] = fs[frame_set].depth[l];
    a.kf_depth = fs[kf].depth[g.top()];
    a.counts = fuse.counts.as<uint8_t>(); a.staged = carry.staged.as<uint8_t>();
    launch_kf_carry(a, stream);
    return true;
}

void Batch::commit_carry()
{
    KfCarryCommitArgs a{};
    a.staged = carry.staged.as<uint8_t>(); a.counts = fuse.counts.as<uint8_t>(); a.table = carry.table.as<KfSeq>();
    a.npix = g.w[g.top()] * g.h[g.top()]; a.n_seq = n_seq;
    launch_kf_carry_commit(a, stream);
}

// ------------------------------------------------------------------------------------------------ keyframe maps as point clouds
int PointsExport::run(const Source& src, const dvo_points_config& cfg, uint32_t capacity, float* xyzg, uint32_t* src_idx, float* sigma_out,
                      uint32_t* offsets_out, hipStream_t s)
{
    const size_t n = (size_t)src.n_seq;
    if (!table.p) {   // (the top level has the most chunks: one allocation serves every level)
        DVO_TRY(table.alloc(sizeof(PointsSeq) * n));
        DVO_TRY(seq_total.alloc(sizeof(uint32_t) * n));
        DVO_TRY(chunk_count.alloc(sizeof(uint32_t) * n * (size_t)points_chunks(src.top_w, src.top_h)));
        DVO_TRY(offsets.alloc(sizeof(uint32_t) * (n + 1)));
    }
    PointsPrepArgs pa{};
    pa.meta = src.meta; pa.started = src.started; pa.started_by_total = src.started_by_total; pa.is_key = src.is_key;
    pa.select_new = cfg.select == DVO_POINTS_NEW ? 1 : 0;
    pa.table = table.as<PointsSeq>(); pa.seq_total = seq_total.as<uint32_t>(); pa.n_seq = src.n_seq;
    launch_points_prep(pa, s);
    PointsArgs a{};
    a.depth = src.depth; a.gray = src.gray; a.sigma = src.sigma;
    a.age = cfg.min_age > 0.0f ? src.age : nullptr;
    a.counts = cfg.min_count > 0 ? src.counts : nullptr;
    a.table = table.as<PointsSeq>(); a.chunk_count = chunk_count.as<uint32_t>(); a.seq_total = seq_total.as<uint32_t>();
    a.offsets = offsets.as<uint32_t>();
    a.xyzg = xyzg; a.src = src_idx; a.sigma_out = sigma_out; a.capacity = capacity;
    a.seq_k = src.seq_k; a.k = src.k;
    a.w = src.w; a.h = src.h; a.n_seq = src.n_seq; a.stride = cfg.stride; a.min_count = cfg.min_count;
    a.gate_sigma = cfg.max_sigma < __builtin_inff() ? 1 : 0;
    a.min_depth = cfg.min_depth; a.max_depth = cfg.max_depth; a.max_sigma = cfg.max_sigma; a.min_age = cfg.min_age;
    launch_points(a, offsets_out, s);
    DVO_HIP(hipGetLastError());
    ready = true;
    return DVO_OK;
}

// the keyframes of a sensor-depth batch with keyframe tracking: fs[cur], kf_meta; no sigma or age maps, the fusion's counts
PointsExport::Source Batch::points_source(int level) const
{
    PointsExport::Source src;
    const FrameSet& F = fs[cur];
    src.meta = kf_meta.as<MonoSeq>(); src.started_by_total = 1; src.is_key = is_key.as<int>();
    src.depth = F.depth[level]; src.gray = F.gray[level];
    src.counts = fuse.ran ? fuse.counts.as<uint8_t>() : nullptr;
    src.seq_k = cam_table() ? cam_table() + (size_t)level * n_seq : nullptr;
    src.k = g.k[level];
    src.w = g.w[level]; src.h = g.h[level]; src.top_w = g.w[g.top()]; src.top_h = g.h[g.top()]; src.n_seq = n_seq;
    return src;
}

// ------------------------------------------------------------------------------------------------ batch: tracking quality records
int TrackQuality::set(bool enable, Tracker& trk, hipStream_t s)
{
    if (enable && !rec.p) {
        DVO_TRY(rec.alloc(sizeof(dvo_gn_result) * (size_t)trk.n_seq));
        DVO_TRY(stage.alloc(sizeof(dvo_track_quality) * (size_t)trk.n_seq));
        DVO_HIP(hipMemsetAsync(rec.p, 0, rec.bytes, s));
    }
    on = enable;
    trk.quality = enable ? rec.as<dvo_gn_result>() : nullptr;
    return DVO_OK;
}

int TrackQuality::launch(const Tracker& trk, const int* status, int all_status, dvo_track_quality* out, hipStream_t s) const
{
    QualityArgs a{};
    a.rec = rec.as<dvo_gn_result>(); a.log = trk.log.as<dvo_track_log>();
    a.status = status; a.all_status = all_status; a.out = out;
    a.levels = trk.g.levels;
    a.max_iterations = trk.cfg.max_iterations; a.fixed_iterations = trk.cfg.fixed_iterations;
    a.min_update = trk.cfg.min_update; a.min_residual = trk.cfg.min_residual;
    a.n_seq = trk.n_seq;
    launch_track_quality(a, s);
    DVO_HIP(hipGetLastError());
    return DVO_OK;
}

int TrackQuality::read_host(const Tracker& trk, const int* status, int all_status, dvo_track_quality* out, hipStream_t s)
{
    DVO_TRY(launch(trk, status, all_status, stage.as<dvo_track_quality>(), s));
    DVO_HIP(hipMemcpyAsync(out, stage.p, stage.bytes, hipMemcpyDeviceToHost, s));
    DVO_HIP(hipStreamSynchronize(s));
    return DVO_OK;
}

}  // namespace dvo
