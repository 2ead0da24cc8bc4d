// dvo_capi.cpp -- the extern "C" surface declared in include/dvo.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <dlfcn.h>
#include <new>
#include <vector>

#include "dvo_engine.h"

using namespace dvo;

struct dvo_vo { VisualOdometry impl; };

extern "C" {

void dvo_config_default(dvo_config* c)
{
    if (!c) return;
    memset(c, 0, sizeof *c);
    c->max_iterations = 15;              // tracker.cpp:19
    c->min_update = 5e-4f;               // tracker.cpp:17
    c->min_residual = 5e-3f;             // tracker.cpp:16
    c->fixed_iterations = 0;
    c->crop_enable = 1;
    c->step_default = 2.0f;              // optimize.cpp:22-26
    c->step_level1 = 1.5f;
    c->step_level2 = 1.0f;
    c->sigma_min = 0.01f;                // optimize.cpp:83
    c->sigma_max = 0.5f;
    c->min_depth = 0.20f;                // optimize.cpp:39
    c->keyframe_min_translation = 0.02f; // mapper.cpp:12
    c->keyframe_max_frames = 6;          // mapper.cpp:13
    c->rng_seed = 0;
    c->device = 0;
    c->stream = nullptr;
    c->profile = 0;
    c->gn_pixels_per_thread = 0;
    c->gn_use_lds_patch = -1;
    c->gn_gather_group = 0;
    c->track_streams = 0;
    c->track_adaptive = 0;
    c->track_fused_tiles = 0;
    c->track_single_launch = 0;
}

const char* dvo_version(void) { return "dvo-mi355x 0.1 (gfx950)"; }

const char* dvo_status_string(int s)
{
    switch (s) {
        case DVO_OK: return "ok";
        case DVO_ERR_BAD_ARGUMENT: return "bad argument";
        case DVO_ERR_HIP: return "HIP runtime error";
        case DVO_ERR_NO_DEVICE: return "no HIP device (libdvo has no CPU fallback)";
        case DVO_ERR_NO_VALID_PIXELS: return "no valid pixels";
        case DVO_ERR_NOT_READY: return "not ready";
        case DVO_ERR_OUT_OF_MEMORY: return "out of device memory";
        default: return "unknown status";
    }
}

const char* dvo_last_error(void) { return last_error(); }

int dvo_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ------------------------------------------------------------------------------------------------ VisualOdometry
int dvo_vo_create(const float K[9], int width, int height, const dvo_config* cfg, dvo_vo** out)
{
    if (!out) return DVO_ERR_BAD_ARGUMENT;
    *out = nullptr;
    dvo_vo* vo = new (std::nothrow) dvo_vo();
    if (!vo) return DVO_ERR_OUT_OF_MEMORY;
    const int st = vo->impl.init(K, width, height, cfg);
    if (st != DVO_OK) { delete vo; return st; }
    *out = vo;
    return DVO_OK;
}

int dvo_vo_destroy(dvo_vo* vo)
{
    if (!vo) return DVO_OK;
    (void)select_device(vo->impl.device);
    if (vo->impl.stream) (void)hipStreamSynchronize(vo->impl.stream);
    delete vo;
    return DVO_OK;
}

int dvo_vo_set_initial_depth(dvo_vo* vo, const float* depth, const float* sigma)
{
    if (!vo || !depth || !sigma) return DVO_ERR_BAD_ARGUMENT;
    const Geometry& g = vo->impl.geoM;
    const size_t n = (size_t)g.w[g.top()] * g.h[g.top()];
    vo->impl.init_depth.assign(depth, depth + n);
    vo->impl.init_sigma.assign(sigma, sigma + n);
    return DVO_OK;
}

int dvo_vo_init_keyframe(dvo_vo* vo, const float* gray, const float* depth, const float* sigma)
{
    if (!vo) return DVO_ERR_BAD_ARGUMENT;
    return vo->impl.init_keyframe(gray, depth, sigma);
}

int dvo_vo_odometrize(dvo_vo* vo, const float* gray, float T_world[16], int* is_keyframe)
{
    if (!vo) return DVO_ERR_BAD_ARGUMENT;
    return vo->impl.odometrize(gray, T_world, is_keyframe);
}

int dvo_vo_odometrize_raw(dvo_vo* vo, const uint8_t* rgb, int channels, float T_world[16], int* is_keyframe)
{
    if (!vo || !rgb) return DVO_ERR_BAD_ARGUMENT;
    return vo->impl.odometrize(nullptr, T_world, is_keyframe, rgb, channels);
}

int dvo_vo_set_distortion(dvo_vo* vo, const float D[5])
{
    if (!vo) return DVO_ERR_BAD_ARGUMENT;
    return vo->impl.set_distortion(D);
}

int dvo_vo_set_photometric(dvo_vo* vo, const float inv_response[256], const float* vignette)
{
    if (!vo) { set_error("dvo_vo_set_photometric: null handle"); return DVO_ERR_BAD_ARGUMENT; }
    return vo->impl.set_photometric(inv_response, vignette);
}

int dvo_vo_odometrize_depth(dvo_vo* vo, const float* gray, const float* depth, const float* sigma, float T_rel[16])
{
    if (!vo) return DVO_ERR_BAD_ARGUMENT;
    return vo->impl.odometrize_depth(gray, depth, sigma, T_rel);
}

int dvo_vo_odometrize_depth_raw(dvo_vo* vo, const uint8_t* rgb, int channels, const uint16_t* depth16, float depth_scale, float T_rel[16])
{
    if (!vo) return DVO_ERR_BAD_ARGUMENT;
    return vo->impl.odometrize_depth_raw(rgb, channels, depth16, depth_scale > 0.0f ? depth_scale : 1.0f / 5000.0f, T_rel);   // (0 = the TUM scale, as the batch entries)
}

int dvo_vo_keyframe_count(const dvo_vo* vo) { return vo ? (int)vo->impl.hist.size() : 0; }

int dvo_vo_keyframe_info(const dvo_vo* vo, int index, int* id, int* levels, int* tw, int* th, float xi[6], float rel_xi[6])
{
    if (!vo || index < 0 || index >= (int)vo->impl.hist.size()) return DVO_ERR_BAD_ARGUMENT;  // frame.hpp:176 .at()
    const Keyframe& k = *vo->impl.hist[index];
    if (id) *id = k.id;
    if (levels) *levels = k.fs.g.levels;
    if (tw) *tw = k.fs.g.w[k.fs.g.top()];
    if (th) *th = k.fs.g.h[k.fs.g.top()];
    if (xi) memcpy(xi, k.xi, 6 * sizeof(float));
    if (rel_xi) memcpy(rel_xi, k.rel_xi, 6 * sizeof(float));
    return DVO_OK;
}

int dvo_vo_keyframe_get(const dvo_vo* vo, int index, int level, float* gray, float* depth, float* sigma, float* age, float K[9])
{
    if (!vo || index < 0 || index >= (int)vo->impl.hist.size()) return DVO_ERR_BAD_ARGUMENT;
    const Keyframe& k = *vo->impl.hist[index];
    if (level < 0 || level >= k.fs.g.levels) return DVO_ERR_BAD_ARGUMENT;  // frame.hpp:125 .at()
    DVO_TRY(select_device(vo->impl.device));
    hipStream_t s = vo->impl.stream;
    const size_t n = (size_t)k.fs.g.w[level] * k.fs.g.h[level] * sizeof(float);
    if (gray) DVO_HIP(hipMemcpyAsync(gray, k.fs.gray[level], n, hipMemcpyDeviceToHost, s));
    if (depth) DVO_HIP(hipMemcpyAsync(depth, k.fs.depth[level], n, hipMemcpyDeviceToHost, s));
    if (sigma) DVO_HIP(hipMemcpyAsync(sigma, k.fs.sigma[level], n, hipMemcpyDeviceToHost, s));
    if (age) {
        if (level != k.fs.g.top()) { set_error("age is stored for the top level only"); return DVO_ERR_BAD_ARGUMENT; }
        DVO_HIP(hipMemcpyAsync(age, k.age.p, n, hipMemcpyDeviceToHost, s));
    }
    if (K) memcpy(K, k.fs.g.K9[level], 9 * sizeof(float));
    DVO_HIP(hipStreamSynchronize(s));
    return DVO_OK;
}

int dvo_vo_last_frame_pose(const dvo_vo* vo, int* id, float xi[6], float rel_xi[6])
{
    if (!vo) return DVO_ERR_BAD_ARGUMENT;
    if (vo->impl.last_id < 0) return DVO_ERR_NOT_READY;
    if (id) *id = vo->impl.last_id;
    if (xi) memcpy(xi, vo->impl.last_xi, 6 * sizeof(float));
    if (rel_xi) memcpy(rel_xi, vo->impl.last_rel, 6 * sizeof(float));
    return DVO_OK;
}

// diagnostic (DVO_PERSIST_TIMELINE=1): wall-clock stamps [2][64][8] of the last k_track_persist launch of the sensor-depth tracker
int dvo_debug_persist_timeline(dvo_vo* vo, long long* out)
{
    if (!vo || !out) return DVO_ERR_BAD_ARGUMENT;
    return vo->impl.trkD.read_persist_timeline(out);
}

int dvo_vo_last_valid_updates(const dvo_vo* vo)
{
    if (!vo) return 0;
    (void)const_cast<dvo_vo*>(vo)->impl.fetch_valid_updates();   // (read back on demand)
    return vo->impl.last_valid_updates;
}

int dvo_vo_last_track_log(const dvo_vo* vo, dvo_track_log* log)
{
    if (!vo || !log) return DVO_ERR_BAD_ARGUMENT;
    DVO_TRY(const_cast<dvo_vo*>(vo)->impl.fetch_log());   // (read back on demand: the record is not part of the per-frame hand-over)
    *log = vo->impl.last_log;
    return DVO_OK;
}

// ------------------------------------------------------------------------------------------------ batch
int dvo_batch_create(int n_seq, const float K[9], int width, int height, int levels, int culls, const dvo_config* cfg, dvo_batch** out)
{
    if (!out) return DVO_ERR_BAD_ARGUMENT;
    *out = nullptr;
    dvo_batch* b = new (std::nothrow) dvo_batch();
    if (!b) return DVO_ERR_OUT_OF_MEMORY;
    const int st = b->impl.init(n_seq, K, width, height, levels, culls, cfg);
    if (st != DVO_OK) { delete b; return st; }
    *out = b;
    return DVO_OK;
}

int dvo_batch_destroy(dvo_batch* b)
{
    if (!b) return DVO_OK;
    (void)select_device(b->device());
    if (b->stream()) (void)hipStreamSynchronize(b->stream());
    delete b;
    return DVO_OK;
}

// a mono batch (dvo_batch_create_mono) has no sensor-depth entry points
#define DVO_NOT_MONO(b)                                                                                   \
    do {                                                                                                  \
        if ((b)->mono) { set_error("this entry point needs a sensor-depth batch (dvo_batch_create)"); return DVO_ERR_BAD_ARGUMENT; } \
    } while (0)

int dvo_batch_push_device(dvo_batch* b, const float* gray, const float* depth, const float* sigma)
{
    if (!b) return DVO_ERR_BAD_ARGUMENT;
    DVO_NOT_MONO(b);
    FrameInput in;
    in.gray = gray; in.depth = depth; in.sigma = sigma;
    return b->impl.push(in);
}

int dvo_batch_prefetch_device(dvo_batch* b, const float* gray, const float* depth, const float* sigma)
{
    if (!b) return DVO_ERR_BAD_ARGUMENT;
    DVO_NOT_MONO(b);
    FrameInput in;
    in.gray = gray; in.depth = depth; in.sigma = sigma;
    return b->impl.prefetch(in);
}

static int raw_input(dvo_batch* b, const uint8_t* rgb, int channels, const uint16_t* depth16, float depth_scale, FrameInput& in)
{
    if (!b || !rgb || !depth16 || (channels != 1 && channels != 3 && channels != 4)) { set_error("bad raw frame"); return DVO_ERR_BAD_ARGUMENT; }
    in.rgb = rgb; in.channels = channels; in.depth16 = depth16; in.depth_scale = depth_scale > 0.0f ? depth_scale : 1.0f / 5000.0f;
    return DVO_OK;
}

int dvo_batch_push_raw_device(dvo_batch* b, const uint8_t* rgb_dev, int channels, const uint16_t* depth16_dev, float depth_scale)
{
    if (!b) return DVO_ERR_BAD_ARGUMENT;
    DVO_NOT_MONO(b);
    FrameInput in;
    DVO_TRY(raw_input(b, rgb_dev, channels, depth16_dev, depth_scale, in));
    return b->impl.push(in);
}

int dvo_batch_prefetch_raw_device(dvo_batch* b, const uint8_t* rgb_dev, int channels, const uint16_t* depth16_dev, float depth_scale)
{
    if (!b) return DVO_ERR_BAD_ARGUMENT;
    DVO_NOT_MONO(b);
    FrameInput in;
    DVO_TRY(raw_input(b, rgb_dev, channels, depth16_dev, depth_scale, in));
    return b->impl.prefetch(in);
}

int dvo_batch_push_raw_host(dvo_batch* b, const uint8_t* rgb, int channels, const uint16_t* depth16, float depth_scale)
{
    if (!b) return DVO_ERR_BAD_ARGUMENT;
    DVO_NOT_MONO(b);
    FrameInput in;
    DVO_TRY(raw_input(b, rgb, channels, depth16, depth_scale, in));
    return b->impl.push_host_frame(rgb, depth16, nullptr, in);
}

int dvo_batch_push_host(dvo_batch* b, const float* gray, const float* depth, const float* sigma)
{
    if (!b || !gray || !depth || !sigma) return DVO_ERR_BAD_ARGUMENT;
    DVO_NOT_MONO(b);
    FrameInput in;
    in.gray = gray; in.depth = depth; in.sigma = sigma;   // (replaced by the staging pointers)
    return b->impl.push_host_frame(gray, depth, sigma, in);
}

int dvo_batch_last_poses(dvo_batch* b, float* xi_rel, float* T_rel)
{
    if (!b) return DVO_ERR_BAD_ARGUMENT;
    DVO_NOT_MONO(b);
    Batch& B = b->impl;
    if (!B.have_poses) return DVO_ERR_NOT_READY;
    DVO_TRY(select_device(B.device));
    if (xi_rel) DVO_HIP(hipMemcpyAsync(xi_rel, B.trk.xi_out.p, sizeof(float) * 6 * (size_t)B.n_seq, hipMemcpyDeviceToHost, B.stream));
    if (T_rel) DVO_HIP(hipMemcpyAsync(T_rel, B.trk.T_out.p, sizeof(float) * 16 * (size_t)B.n_seq, hipMemcpyDeviceToHost, B.stream));
    DVO_HIP(hipStreamSynchronize(B.stream));
    return DVO_OK;
}

int dvo_batch_copy_poses_device(dvo_batch* b, float* xi_dst_dev, float* T_dst_dev)
{
    if (!b) return DVO_ERR_BAD_ARGUMENT;
    DVO_NOT_MONO(b);
    Batch& B = b->impl;
    if (!B.have_poses) return DVO_ERR_NOT_READY;
    DVO_TRY(select_device(B.device));
    if (xi_dst_dev) DVO_HIP(hipMemcpyAsync(xi_dst_dev, B.trk.xi_out.p, sizeof(float) * 6 * (size_t)B.n_seq, hipMemcpyDeviceToDevice, B.stream));
    if (T_dst_dev) DVO_HIP(hipMemcpyAsync(T_dst_dev, B.trk.T_out.p, sizeof(float) * 16 * (size_t)B.n_seq, hipMemcpyDeviceToDevice, B.stream));
    return DVO_OK;
}

int dvo_batch_last_track_log(dvo_batch* b, int seq, dvo_track_log* log)
{
    if (!b || !log || seq < 0) return DVO_ERR_BAD_ARGUMENT;
    if (seq >= b->n_seq()) return DVO_ERR_BAD_ARGUMENT;
    // (a mono batch: the log of the last tracked frame, so not before the second call)
    if (b->mono ? b->mono->latest_id < 1 : !b->impl.have_poses) return DVO_ERR_NOT_READY;
    DVO_TRY(select_device(b->device()));
    DVO_HIP(hipMemcpyAsync(log, b->trk().log.as<dvo_track_log>() + seq, sizeof *log, hipMemcpyDeviceToHost, b->stream()));
    DVO_HIP(hipStreamSynchronize(b->stream()));
    return DVO_OK;
}

// diagnostic, read-only: Tracker::lv[level] as use_plan() left it -- what the next push / call launches on that level
int dvo_debug_batch_level_plan(dvo_batch* b, int level, int* ppt, int* group, int* tiles_2d, int* tiles, int* schedule)
{
    if (!b) return DVO_ERR_BAD_ARGUMENT;
    const Tracker& T = b->trk();
    if (level < 0 || level >= T.g.levels) return DVO_ERR_BAD_ARGUMENT;
    const LevelPlan& L = T.lv[level];
    if (ppt) *ppt = L.ppt;
    if (group) *group = L.group;
    if (tiles_2d) *tiles_2d = L.tiling.t2d ? 1 : 0;   // (the LDS-patch schedule leaves the default tiling: not 2-D)
    if (tiles) *tiles = L.nblk;
    if (schedule) *schedule = L.schedule;
    return DVO_OK;
}

int dvo_batch_frame_get(dvo_batch* b, int seq, int level, float* gray, float* depth)
{
    if (!b) return DVO_ERR_BAD_ARGUMENT;
    DVO_NOT_MONO(b);
    Batch& B = b->impl;
    if (seq < 0 || seq >= B.n_seq || level < 0 || level >= B.g.levels) return DVO_ERR_BAD_ARGUMENT;
    if (B.cur < 0) return DVO_ERR_NOT_READY;
    DVO_TRY(select_device(B.device));
    // (in stream order after the push, which has queued the wait for a split build's side stream)
    // keyframe tracking: fs[cur] holds the keyframes; the last push's frame is in fs[prev] (the first push's frame is the keyframe)
    const FrameSet& F = B.fs[(B.kf_on && B.prev >= 0) ? B.prev : B.cur];
    const size_t n = (size_t)B.g.w[level] * B.g.h[level], off = n * (size_t)seq;
    if (gray) DVO_HIP(hipMemcpyAsync(gray, F.gray[level] + off, n * 4, hipMemcpyDeviceToHost, B.stream));
    if (depth) DVO_HIP(hipMemcpyAsync(depth, F.depth[level] + off, n * 4, hipMemcpyDeviceToHost, B.stream));
    DVO_HIP(hipStreamSynchronize(B.stream));
    return DVO_OK;
}

int dvo_batch_synchronize(dvo_batch* b)
{
    if (!b) return DVO_ERR_BAD_ARGUMENT;
    DVO_TRY(select_device(b->device()));
    DVO_HIP(hipStreamSynchronize(b->stream()));
    return DVO_OK;
}

int dvo_batch_set_actions(dvo_batch* b, const uint8_t* actions, int actions_on_device)
{
    if (!b) return DVO_ERR_BAD_ARGUMENT;
    if (b->mono) { set_error("dvo_batch_set_actions: a mono batch advances in lockstep (per-sequence actions need dvo_batch_create)"); return DVO_ERR_BAD_ARGUMENT; }
    return b->impl.set_actions(actions, actions_on_device != 0);
}

int dvo_batch_set_pose_guess_mode(dvo_batch* b, int mode)
{
    if (!b) return DVO_ERR_BAD_ARGUMENT;
    if (mode != DVO_GUESS_NONE && mode != DVO_GUESS_GIVEN && mode != DVO_GUESS_CONSTANT_VELOCITY) {
        set_error("dvo_batch_set_pose_guess_mode: the mode is DVO_GUESS_NONE, DVO_GUESS_GIVEN or DVO_GUESS_CONSTANT_VELOCITY");
        return DVO_ERR_BAD_ARGUMENT;
    }
    return b->mono ? b->mono->set_guess_mode(mode) : b->impl.set_guess_mode(mode);
}

int dvo_batch_set_keyframe_tracking(dvo_batch* b, int enable)
{
    if (!b) return DVO_ERR_BAD_ARGUMENT;
    if (b->mono) { set_error("dvo_batch_set_keyframe_tracking: needs a sensor-depth batch (a mono batch always tracks against keyframes)"); return DVO_ERR_BAD_ARGUMENT; }
    return b->impl.set_keyframe_tracking(enable);
}

void dvo_kf_fusion_config_default(dvo_kf_fusion_config* cfg)
{
    if (!cfg) return;
    cfg->mode = DVO_KF_FUSION_ON;
    cfg->max_diff = 0.05f;
    cfg->max_count = 16;
}

// the checks every keyframe-fusion entry point shares: a sensor-depth batch with keyframe tracking
static int kf_fusion_handle_ok(dvo_batch* b, const char* who)
{
    if (!b) return DVO_ERR_BAD_ARGUMENT;
    if (b->mono) { set_error(std::string(who) + ": needs a sensor-depth batch (a mono batch refines its keyframe maps itself)"); return DVO_ERR_BAD_ARGUMENT; }
    if (!b->impl.kf_on) { set_error(std::string(who) + ": keyframe tracking is off (dvo_batch_set_keyframe_tracking)"); return DVO_ERR_NOT_READY; }
    return DVO_OK;
}

static int kf_max_diff_ok(float max_diff, const char* who)
{
    if (!(max_diff > 0.0f && max_diff < __builtin_inff())) { set_error(std::string(who) + ": max_diff must be finite and > 0"); return DVO_ERR_BAD_ARGUMENT; }
    return DVO_OK;
}

int dvo_batch_set_keyframe_fusion(dvo_batch* b, const dvo_kf_fusion_config* cfg)
{
    static const char who[] = "dvo_batch_set_keyframe_fusion";
    DVO_TRY(kf_fusion_handle_ok(b, who));
    if (cfg) {
        if (cfg->mode != DVO_KF_FUSION_OFF && cfg->mode != DVO_KF_FUSION_ON) { set_error(std::string(who) + ": the mode is DVO_KF_FUSION_OFF or DVO_KF_FUSION_ON"); return DVO_ERR_BAD_ARGUMENT; }
        DVO_TRY(kf_max_diff_ok(cfg->max_diff, who));
        if (cfg->max_count < 1 || cfg->max_count > 255) { set_error(std::string(who) + ": max_count must be in [1, 255]"); return DVO_ERR_BAD_ARGUMENT; }
    }
    return b->impl.set_keyframe_fusion(cfg);
}

// dvo_batch_last_keyframe_fusion / _carry: the stage's records of the last push as the public record type, whose middle counter is `done`
extern "C++" template <class Rec>
static int kf_last_records(Batch& B, const Batch::KfStage& st, const char* who, const char* not_ready, Rec* rec, int Rec::*done)
{
    if (!st.ready) { set_error(std::string(who) + not_ready); return DVO_ERR_NOT_READY; }
    DVO_TRY(select_device(B.device));
    std::vector<KfRecord> host((size_t)B.n_seq);
    DVO_HIP(hipMemcpyAsync(host.data(), st.rec.p, sizeof(KfRecord) * host.size(), hipMemcpyDeviceToHost, B.stream));
    DVO_HIP(hipStreamSynchronize(B.stream));
    for (size_t i = 0; i < host.size(); i++) {
        rec[i].struct_size = (int)sizeof(Rec);
        rec[i].n_candidates = host[i].n_candidates; rec[i].*done = host[i].n_done; rec[i].n_gated = host[i].n_gated;
    }
    return DVO_OK;
}

int dvo_batch_last_keyframe_fusion(dvo_batch* b, dvo_kf_fusion_record* rec)
{
    static const char who[] = "dvo_batch_last_keyframe_fusion";
    if (!rec) return DVO_ERR_BAD_ARGUMENT;
    DVO_TRY(kf_fusion_handle_ok(b, who));
    return kf_last_records(b->impl, b->impl.fuse, who, ": the last push did not run with keyframe fusion (dvo_batch_set_keyframe_fusion)", rec,
                           &dvo_kf_fusion_record::n_fused);
}

int dvo_batch_keyframe_fusion_counts(dvo_batch* b, int seq, uint8_t* counts)
{
    static const char who[] = "dvo_batch_keyframe_fusion_counts";
    if (!counts) return DVO_ERR_BAD_ARGUMENT;
    DVO_TRY(kf_fusion_handle_ok(b, who));
    Batch& B = b->impl;
    if (seq < 0 || seq >= B.n_seq) { set_error(std::string(who) + ": seq is out of range"); return DVO_ERR_BAD_ARGUMENT; }
    if (!B.fuse.ran) { set_error(std::string(who) + ": no push has run with keyframe fusion yet (dvo_batch_set_keyframe_fusion)"); return DVO_ERR_NOT_READY; }
    DVO_TRY(select_device(B.device));
    const size_t n = (size_t)B.g.w[B.g.top()] * B.g.h[B.g.top()];
    DVO_HIP(hipMemcpyAsync(counts, B.fuse.counts.as<uint8_t>() + n * (size_t)seq, n, hipMemcpyDeviceToHost, B.stream));
    DVO_HIP(hipStreamSynchronize(B.stream));
    return DVO_OK;
}

void dvo_kf_carry_config_default(dvo_kf_carry_config* cfg)
{
    if (!cfg) return;
    cfg->struct_size = (int)sizeof(dvo_kf_carry_config);
    cfg->mode = DVO_KF_CARRY_ON;
    cfg->max_diff = 0.05f;
}

// the checks both keyframe-carry entry points share: a sensor-depth batch with keyframe tracking and fusion on
static int kf_carry_handle_ok(dvo_batch* b, const char* who)
{
    DVO_TRY(kf_fusion_handle_ok(b, who));
    if (!b->impl.fuse.on) { set_error(std::string(who) + ": keyframe fusion is off (dvo_batch_set_keyframe_fusion)"); return DVO_ERR_NOT_READY; }
    return DVO_OK;
}

int dvo_batch_set_keyframe_carry(dvo_batch* b, const dvo_kf_carry_config* cfg)
{
    static const char who[] = "dvo_batch_set_keyframe_carry";
    DVO_TRY(kf_carry_handle_ok(b, who));
    if (cfg) {
        if (cfg->struct_size != (int)sizeof(dvo_kf_carry_config)) { set_error(std::string(who) + ": struct_size is not sizeof(dvo_kf_carry_config)"); return DVO_ERR_BAD_ARGUMENT; }
        if (cfg->mode != DVO_KF_CARRY_OFF && cfg->mode != DVO_KF_CARRY_ON) { set_error(std::string(who) + ": the mode is DVO_KF_CARRY_OFF or DVO_KF_CARRY_ON"); return DVO_ERR_BAD_ARGUMENT; }
        DVO_TRY(kf_max_diff_ok(cfg->max_diff, who));
    }
    return b->impl.set_keyframe_carry(cfg);
}

int dvo_batch_last_keyframe_carry(dvo_batch* b, dvo_kf_carry_record* rec)
{
    static const char who[] = "dvo_batch_last_keyframe_carry";
    if (!rec) return DVO_ERR_BAD_ARGUMENT;
    DVO_TRY(kf_carry_handle_ok(b, who));
    return kf_last_records(b->impl, b->impl.carry, who, ": the last push did not run with keyframe carry (dvo_batch_set_keyframe_carry)", rec,
                           &dvo_kf_carry_record::n_carried);
}

int dvo_batch_set_pose_guess(dvo_batch* b, const float* xi, int xi_on_device)
{
    if (!b) return DVO_ERR_BAD_ARGUMENT;
    PoseGuess& G = b->guess();
    if (xi && G.mode != DVO_GUESS_GIVEN) { set_error("dvo_batch_set_pose_guess: rows need the mode DVO_GUESS_GIVEN"); return DVO_ERR_BAD_ARGUMENT; }
    DVO_TRY(select_device(b->device()));
    return G.given.set(xi, xi_on_device != 0, sizeof(float) * 6 * (size_t)b->n_seq(), b->stream());
}

int dvo_batch_last_start_poses(dvo_batch* b, float* xi_start)
{
    if (!b || !xi_start) return DVO_ERR_BAD_ARGUMENT;
    if (b->pushes() == 0) { set_error("dvo_batch_last_start_poses: nothing has been pushed yet"); return DVO_ERR_NOT_READY; }
    DVO_TRY(select_device(b->device()));
    const PoseGuess& G = b->guess();
    if (!G.on()) {   // no mode was ever set: every push started from zero
        DVO_HIP(hipStreamSynchronize(b->stream()));
        memset(xi_start, 0, sizeof(float) * 6 * (size_t)b->n_seq());
        return DVO_OK;
    }
    return G.last_start(xi_start, b->stream());
}

int dvo_batch_set_track_quality(dvo_batch* b, int enable)
{
    if (!b) return DVO_ERR_BAD_ARGUMENT;
    DVO_TRY(select_device(b->device()));
    return b->quality().set(enable != 0, b->trk(), b->stream());
}

// the records of the last push / call: its status (per-sequence path: the device status k_plan wrote; plain pushes: all STARTED on the
// first, all TRACKED after), launched on the handle's stream into `out` (device) or, with to_host, through the staging buffer
static int track_quality(dvo_batch* b, dvo_track_quality* out, bool to_host)
{
    if (!b || !out) return DVO_ERR_BAD_ARGUMENT;
    TrackQuality& Q = b->quality();
    if (!Q.ready) { set_error("dvo_batch_last_track_quality: the last push / call did not keep quality records (dvo_batch_set_track_quality)"); return DVO_ERR_NOT_READY; }
    DVO_TRY(select_device(b->device()));
    const int* status = b->plan().act_used ? b->plan().status.as<int>() : nullptr;
    const int all = b->pushes() == 1 ? DVO_SEQ_STARTED : DVO_SEQ_TRACKED;
    return to_host ? Q.read_host(b->trk(), status, all, out, b->stream()) : Q.launch(b->trk(), status, all, out, b->stream());
}

int dvo_batch_last_track_quality(dvo_batch* b, dvo_track_quality* out) { return track_quality(b, out, true); }
int dvo_batch_copy_track_quality_device(dvo_batch* b, dvo_track_quality* dst) { return track_quality(b, dst, false); }

// ------------------------------------------------------------------------------------------------ batch: the opt-in tracking terms
// Which terms combine is the engine's table (Tracker::refusal): the setters validate their configuration and hand it
// over with their own name, which the refusal's message starts with.

// What every dvo_batch_last_* reader of a term checks before it reads, in this order: the handle, the output and (log readers) the
// sequence; the caller's struct_size (log readers: want_size and the type's name); that the last push / call ran with the term, else
// DVO_ERR_NOT_READY naming the term and its setter; the device.
static int reader_begin(dvo_batch* b, const void* out, const char* who, Term term, int seq = 0, int struct_size = 0, size_t want_size = 0,
                        const char* type = "")
{
    if (!b || !out || seq < 0 || seq >= b->n_seq()) return DVO_ERR_BAD_ARGUMENT;
    if (struct_size != (int)want_size) { set_error(std::string(who) + ": struct_size is not sizeof(" + type + ")"); return DVO_ERR_BAD_ARGUMENT; }
    const Tracker& t = b->trk();
    bool ready = false;
    const char* with = "";
    switch (term) {
    case TERM_ROBUST:       ready = t.rob.ready;        with = "robust weights (dvo_batch_set_robust_weights)"; break;
    case TERM_MEDIAN:       ready = t.rob.median_ready; with = "the median robust scale (dvo_batch_set_robust_median)"; break;
    case TERM_AFFINE:       ready = t.aff.ready;        with = "affine brightness compensation (dvo_batch_set_affine_brightness)"; break;
    case TERM_GEOMETRIC:    ready = t.geo.ready;        with = "the geometric term (dvo_batch_set_geometric)"; break;
    case TERM_STEP_CONTROL: ready = t.lm.ready;         with = "step control (dvo_batch_set_step_control)"; break;
    }
    if (!ready) { set_error(std::string(who) + ": the last push / call did not run with " + with); return DVO_ERR_NOT_READY; }
    return select_device(b->device());
}
#define DVO_LOG_READER(b, log, who, term, seq, type) reader_begin(b, log, who, term, seq, (log) ? (log)->struct_size : 0, sizeof(type), #type)

// kind and param of robust weights, wherever they come from (a dvo_robust_config, the arguments of the dvo_op_gn_step_* operators)
static bool robust_kind_param_ok(const char* who, int kind, float param)
{
    if (kind != DVO_ROBUST_NONE && kind != DVO_ROBUST_HUBER && kind != DVO_ROBUST_STUDENT_T) {
        set_error(std::string(who) + ": the kind is DVO_ROBUST_NONE, DVO_ROBUST_HUBER or DVO_ROBUST_STUDENT_T");
        return false;
    }
    if (kind != DVO_ROBUST_NONE && !(param > 0.0f && param < __builtin_inff())) {
        set_error(std::string(who) + ": param (Huber k, Student-t nu) must be finite and > 0");
        return false;
    }
    return true;
}

// The checks of a robust configuration (dvo_batch_set_robust_weights, and with `median` dvo_batch_set_robust_median, whose only scale
// mode is DVO_ROBUST_SCALE_MEDIAN and which has no kind NONE)
static bool robust_config_ok(const dvo_robust_config* cfg, const char* who, bool median)
{
    if (cfg->struct_size != (int)sizeof(dvo_robust_config)) { set_error(std::string(who) + ": struct_size is not sizeof(dvo_robust_config)"); return false; }
    if (median && cfg->kind != DVO_ROBUST_HUBER && cfg->kind != DVO_ROBUST_STUDENT_T) {
        set_error(std::string(who) + ": the kind is DVO_ROBUST_HUBER or DVO_ROBUST_STUDENT_T");
        return false;
    }
    if (!robust_kind_param_ok(who, cfg->kind, cfg->param)) return false;
    if (cfg->kind == DVO_ROBUST_NONE) return true;
    if (median && cfg->scale_mode != DVO_ROBUST_SCALE_MEDIAN) {
        set_error(std::string(who) + ": the scale mode is DVO_ROBUST_SCALE_MEDIAN");
        return false;
    }
    if (!median && cfg->scale_mode != DVO_ROBUST_SCALE_ADAPTIVE && cfg->scale_mode != DVO_ROBUST_SCALE_GIVEN) {
        set_error(std::string(who) + ": the scale mode is DVO_ROBUST_SCALE_ADAPTIVE or DVO_ROBUST_SCALE_GIVEN");
        return false;
    }
    if (!(cfg->scale_floor > 0.0f && cfg->scale_floor < __builtin_inff())) {   // (whatever the mode: a configuration is valid or not as a whole)
        set_error(std::string(who) + ": scale_floor must be finite and > 0");
        return false;
    }
    return true;
}

int dvo_batch_set_robust_median(dvo_batch* b, const dvo_robust_config* cfg)
{
    static const char who[] = "dvo_batch_set_robust_median";
    if (!b) return DVO_ERR_BAD_ARGUMENT;
    if (cfg && !robust_config_ok(cfg, who, true)) return DVO_ERR_BAD_ARGUMENT;
    DVO_TRY(select_device(b->device()));
    return b->trk().set_robust(who, cfg, b->stream());
}

int dvo_batch_last_robust_log(dvo_batch* b, int seq, dvo_robust_log* log)
{
    DVO_TRY(DVO_LOG_READER(b, log, "dvo_batch_last_robust_log", TERM_MEDIAN, seq, dvo_robust_log));
    return b->trk().last_robust_log(seq, log, b->stream());
}

int dvo_batch_last_robust_histogram(dvo_batch* b, int seq, uint32_t counts[256])
{
    DVO_TRY(reader_begin(b, counts, "dvo_batch_last_robust_histogram", TERM_MEDIAN, seq));
    return b->trk().last_robust_histogram(seq, counts, b->stream());
}

int dvo_batch_set_robust_weights(dvo_batch* b, const dvo_robust_config* cfg)
{
    static const char who[] = "dvo_batch_set_robust_weights";
    if (!b) return DVO_ERR_BAD_ARGUMENT;
    if (cfg && !robust_config_ok(cfg, who, false)) return DVO_ERR_BAD_ARGUMENT;
    DVO_TRY(select_device(b->device()));
    return b->trk().set_robust(who, cfg, b->stream());
}

int dvo_batch_set_robust_scales(dvo_batch* b, const float* s, int s_on_device)
{
    if (!b) return DVO_ERR_BAD_ARGUMENT;
    RobustWeights& R = b->trk().rob;
    if (s && !(R.on && R.mode == DVO_ROBUST_SCALE_GIVEN)) { set_error("dvo_batch_set_robust_scales: rows need the scale mode DVO_ROBUST_SCALE_GIVEN"); return DVO_ERR_BAD_ARGUMENT; }
    DVO_TRY(select_device(b->device()));
    return R.scales.set(s, s_on_device != 0, sizeof(float) * (size_t)b->n_seq(), b->stream());
}

int dvo_batch_last_robust_scales(dvo_batch* b, float* s2)
{
    DVO_TRY(reader_begin(b, s2, "dvo_batch_last_robust_scales", TERM_ROBUST));
    return b->trk().last_robust_scales(s2, b->stream());
}

// the guards of the next (a, b) entry where no configuration sets them: the operators', and the bindings' defaults
static dvo_affine_config affine_config_given()
{
    dvo_affine_config ac{};
    ac.struct_size = (int)sizeof ac;
    ac.mode = DVO_AFFINE_GIVEN; ac.min_pixels = 64; ac.min_contrast = 1e-3f; ac.gain_min = 0.25f; ac.gain_max = 4.0f;
    return ac;
}

static bool affine_config_ok(const dvo_affine_config* cfg, const char* who)
{
    const auto finite = [](float v) { return v > -__builtin_inff() && v < __builtin_inff(); };
    if (cfg->struct_size != (int)sizeof(dvo_affine_config)) { set_error(std::string(who) + ": struct_size is not sizeof(dvo_affine_config)"); return false; }
    if (cfg->mode != DVO_AFFINE_OFF && cfg->mode != DVO_AFFINE_ESTIMATE && cfg->mode != DVO_AFFINE_GIVEN) {
        set_error(std::string(who) + ": the mode is DVO_AFFINE_OFF, DVO_AFFINE_ESTIMATE or DVO_AFFINE_GIVEN");
        return false;
    }
    if (cfg->mode == DVO_AFFINE_OFF) return true;
    if (cfg->min_pixels < 2) { set_error(std::string(who) + ": min_pixels must be >= 2"); return false; }
    if (!(cfg->min_contrast >= 0.0f && cfg->min_contrast < 1.0f)) { set_error(std::string(who) + ": min_contrast must be in [0, 1)"); return false; }
    if (!(cfg->gain_min > 0.0f) || !finite(cfg->gain_max) || !(cfg->gain_min <= cfg->gain_max)) {
        set_error(std::string(who) + ": the gain range needs 0 < gain_min <= gain_max < inf");
        return false;
    }
    return true;
}

int dvo_batch_set_affine_brightness(dvo_batch* b, const dvo_affine_config* cfg)
{
    static const char who[] = "dvo_batch_set_affine_brightness";
    if (!b) return DVO_ERR_BAD_ARGUMENT;
    if (cfg && !affine_config_ok(cfg, who)) return DVO_ERR_BAD_ARGUMENT;
    DVO_TRY(select_device(b->device()));
    return b->trk().set_affine(who, cfg, b->stream());
}

int dvo_batch_set_affine_rows(dvo_batch* b, const float* ab, int ab_on_device)
{
    if (!b) return DVO_ERR_BAD_ARGUMENT;
    AffineBrightness& A = b->trk().aff;
    if (ab && !(A.on && A.mode == DVO_AFFINE_GIVEN)) { set_error("dvo_batch_set_affine_rows: rows need the mode DVO_AFFINE_GIVEN"); return DVO_ERR_BAD_ARGUMENT; }
    DVO_TRY(select_device(b->device()));
    return A.rows.set(ab, ab_on_device != 0, sizeof(float) * 2 * (size_t)b->n_seq(), b->stream());
}

int dvo_batch_last_affine(dvo_batch* b, float* ab)
{
    DVO_TRY(reader_begin(b, ab, "dvo_batch_last_affine", TERM_AFFINE));
    return b->trk().last_affine(ab, b->stream());
}

int dvo_batch_last_affine_log(dvo_batch* b, int seq, dvo_affine_log* log)
{
    DVO_TRY(DVO_LOG_READER(b, log, "dvo_batch_last_affine_log", TERM_AFFINE, seq, dvo_affine_log));
    return b->trk().last_affine_log(seq, log, b->stream());
}

void dvo_geometric_config_default(dvo_geometric_config* cfg)
{
    if (!cfg) return;
    cfg->struct_size = (int)sizeof(dvo_geometric_config);
    cfg->mode = DVO_GEOMETRIC_ON;
    cfg->weight = 10.0f;
    cfg->max_diff = 0.1f;
}

static bool geometric_config_ok(const dvo_geometric_config* cfg, const char* who)
{
    const float inf = __builtin_inff();
    if (cfg->struct_size != (int)sizeof(dvo_geometric_config)) { set_error(std::string(who) + ": struct_size is not sizeof(dvo_geometric_config)"); return false; }
    if (cfg->mode != DVO_GEOMETRIC_OFF && cfg->mode != DVO_GEOMETRIC_ON) { set_error(std::string(who) + ": the mode is DVO_GEOMETRIC_OFF or DVO_GEOMETRIC_ON"); return false; }
    if (cfg->mode == DVO_GEOMETRIC_OFF) return true;
    if (!(cfg->weight >= 0.0f && cfg->weight < inf)) { set_error(std::string(who) + ": weight must be finite and >= 0"); return false; }
    if (!(cfg->max_diff > 0.0f && cfg->max_diff < inf)) { set_error(std::string(who) + ": max_diff must be finite and > 0"); return false; }
    return true;
}

int dvo_batch_set_geometric(dvo_batch* b, const dvo_geometric_config* cfg)
{
    static const char who[] = "dvo_batch_set_geometric";
    if (!b) return DVO_ERR_BAD_ARGUMENT;
    if (b->mono) { set_error(std::string(who) + ": needs a sensor-depth batch (a mono batch has no depth map to compare)"); return DVO_ERR_BAD_ARGUMENT; }
    if (cfg && !geometric_config_ok(cfg, who)) return DVO_ERR_BAD_ARGUMENT;
    DVO_TRY(select_device(b->device()));
    return b->trk().set_geometric(who, cfg, b->stream());
}

int dvo_batch_set_geometric_affine(dvo_batch* b, const dvo_geometric_config* geo, const dvo_affine_config* aff)
{
    static const char who[] = "dvo_batch_set_geometric_affine";
    if (!b || !geo || !aff) return DVO_ERR_BAD_ARGUMENT;
    if (b->mono) { set_error(std::string(who) + ": needs a sensor-depth batch (a mono batch has no depth map to compare)"); return DVO_ERR_BAD_ARGUMENT; }
    if (!geometric_config_ok(geo, who) || !affine_config_ok(aff, who)) return DVO_ERR_BAD_ARGUMENT;
    if (geo->mode != DVO_GEOMETRIC_ON) { set_error(std::string(who) + ": the geometric mode must be DVO_GEOMETRIC_ON (dvo_batch_set_geometric turns the term off)"); return DVO_ERR_BAD_ARGUMENT; }
    if (aff->mode == DVO_AFFINE_OFF) { set_error(std::string(who) + ": the affine mode must be DVO_AFFINE_ESTIMATE or DVO_AFFINE_GIVEN (dvo_batch_set_affine_brightness turns the compensation off)"); return DVO_ERR_BAD_ARGUMENT; }
    DVO_TRY(select_device(b->device()));
    return b->trk().set_geometric_affine(who, geo, aff, b->stream());
}

int dvo_batch_last_geometric(dvo_batch* b, dvo_geometric_record* rec)
{
    DVO_TRY(reader_begin(b, rec, "dvo_batch_last_geometric", TERM_GEOMETRIC));
    return b->trk().last_geometric(rec, b->stream());
}

int dvo_batch_last_geometric_log(dvo_batch* b, int seq, dvo_geometric_log* log)
{
    DVO_TRY(DVO_LOG_READER(b, log, "dvo_batch_last_geometric_log", TERM_GEOMETRIC, seq, dvo_geometric_log));
    return b->trk().last_geometric_log(seq, log, b->stream());
}

void dvo_lm_config_default(dvo_lm_config* cfg)
{
    if (!cfg) return;
    cfg->struct_size = (int)sizeof(dvo_lm_config);
    cfg->mode = DVO_LM_ON;
    cfg->lambda0 = 1.0f;
    cfg->lambda_up = 4.0f;
    cfg->lambda_down = 0.5f;
    cfg->lambda_floor = 1e-4f;
    cfg->lambda_max = 1e6f;
    cfg->min_valid_fraction = 0.5f;
}

static bool lm_config_ok(const dvo_lm_config* cfg, const char* who)
{
    const float inf = __builtin_inff();
    const auto bad = [&](const char* what) { set_error(std::string(who) + ": " + what); return false; };
    if (cfg->struct_size != (int)sizeof(dvo_lm_config)) return bad("struct_size is not sizeof(dvo_lm_config)");
    if (cfg->mode != DVO_LM_OFF && cfg->mode != DVO_LM_ON) return bad("the mode is DVO_LM_OFF or DVO_LM_ON");
    if (cfg->mode == DVO_LM_OFF) return true;
    if (!(cfg->lambda0 >= 0.0f && cfg->lambda0 < inf)) return bad("lambda0 must be finite and >= 0");
    if (!(cfg->lambda_up > 1.0f && cfg->lambda_up < inf)) return bad("lambda_up must be finite and > 1");
    if (!(cfg->lambda_down > 0.0f && cfg->lambda_down <= 1.0f)) return bad("lambda_down must be in (0, 1]");
    if (!(cfg->lambda_floor > 0.0f && cfg->lambda_floor < inf)) return bad("lambda_floor must be finite and > 0");
    if (!(cfg->lambda_max >= cfg->lambda_floor && cfg->lambda_max < inf)) return bad("lambda_max must be finite and >= lambda_floor");
    if (!(cfg->min_valid_fraction >= 0.0f && cfg->min_valid_fraction <= 1.0f)) return bad("min_valid_fraction must be in [0, 1]");
    return true;
}

int dvo_batch_set_step_control(dvo_batch* b, const dvo_lm_config* cfg)
{
    static const char who[] = "dvo_batch_set_step_control";
    if (!b) return DVO_ERR_BAD_ARGUMENT;
    if (cfg && !lm_config_ok(cfg, who)) return DVO_ERR_BAD_ARGUMENT;
    DVO_TRY(select_device(b->device()));
    return b->trk().set_step_control(who, cfg, b->stream());
}

int dvo_batch_last_step_control(dvo_batch* b, dvo_lm_record* rec)
{
    DVO_TRY(reader_begin(b, rec, "dvo_batch_last_step_control", TERM_STEP_CONTROL));
    return b->trk().last_step_control(rec, b->stream());
}

int dvo_batch_last_step_control_log(dvo_batch* b, int seq, dvo_lm_log* log)
{
    DVO_TRY(DVO_LOG_READER(b, log, "dvo_batch_last_step_control_log", TERM_STEP_CONTROL, seq, dvo_lm_log));
    return b->trk().last_step_control_log(seq, log, b->stream());
}

int dvo_batch_set_intrinsics(dvo_batch* b, const float* K)
{
    if (!b) return DVO_ERR_BAD_ARGUMENT;
    if (b->mono) { set_error("dvo_batch_set_intrinsics: a mono batch has one K (per-sequence intrinsics need dvo_batch_create)"); return DVO_ERR_BAD_ARGUMENT; }
    return b->impl.set_intrinsics(K);
}

int dvo_batch_get_intrinsics(dvo_batch* b, float* K)
{
    if (!b || !K) return DVO_ERR_BAD_ARGUMENT;
    DVO_NOT_MONO(b);
    memcpy(K, b->impl.cam_K.data(), sizeof(float) * b->impl.cam_K.size());
    return DVO_OK;
}

int dvo_batch_set_sensor_distortion(dvo_batch* b, const float* D, int per_sequence)
{
    if (!b) return DVO_ERR_BAD_ARGUMENT;
    if (b->mono) { set_error("dvo_batch_set_sensor_distortion: needs a sensor-depth batch (a mono batch takes D through dvo_batch_set_distortion)"); return DVO_ERR_BAD_ARGUMENT; }
    return b->impl.set_sensor_distortion(D, per_sequence != 0);
}

int dvo_batch_set_pyramid_filter(dvo_batch* b, int filter)
{
    if (!b) return DVO_ERR_BAD_ARGUMENT;
    if (b->mono) { set_error("dvo_batch_set_pyramid_filter: needs a sensor-depth batch"); return DVO_ERR_BAD_ARGUMENT; }
    return b->impl.set_pyramid_filter(filter);
}

int dvo_batch_pyramid_filter(dvo_batch* b, int* filter)
{
    if (!b || !filter) return DVO_ERR_BAD_ARGUMENT;
    if (b->mono) { set_error("dvo_batch_pyramid_filter: needs a sensor-depth batch"); return DVO_ERR_BAD_ARGUMENT; }
    *filter = b->impl.pyr_filter;
    return DVO_OK;
}

int dvo_batch_get_sensor_distortion(dvo_batch* b, float* D, int* enabled)
{
    if (!b) return DVO_ERR_BAD_ARGUMENT;
    DVO_NOT_MONO(b);
    const Undistortion& u = b->impl.und;
    if (D) {
        if (u.enabled()) memcpy(D, u.D.data(), sizeof(float) * u.D.size());
        else memset(D, 0, sizeof(float) * 5 * (size_t)b->impl.n_seq);
    }
    if (enabled) *enabled = u.enabled() ? 1 : 0;
    return DVO_OK;
}

int dvo_batch_last_status(dvo_batch* b, int* status)
{
    if (!b || !status) return DVO_ERR_BAD_ARGUMENT;
    DVO_NOT_MONO(b);
    return b->impl.status_of_last(status, false);
}

int dvo_batch_copy_status_device(dvo_batch* b, int* status_dev)
{
    if (!b || !status_dev) return DVO_ERR_BAD_ARGUMENT;
    DVO_NOT_MONO(b);
    return b->impl.status_of_last(status_dev, true);
}

int dvo_shard_range(int n_sequences, int world_size, int rank, int* first, int* count)
{
    if (n_sequences < 0 || world_size < 1 || rank < 0 || rank >= world_size || !first || !count) return DVO_ERR_BAD_ARGUMENT;
    const int base = n_sequences / world_size, extra = n_sequences % world_size;
    *count = base + (rank < extra ? 1 : 0);
    *first = rank * base + (rank < extra ? rank : extra);
    return DVO_OK;
}

int dvo_batch_gather_poses_rccl(dvo_batch* b, void* rccl_comm, int world_size, float* xi_all_dev)
{
    if (!b || !rccl_comm || world_size < 1 || !xi_all_dev) return DVO_ERR_BAD_ARGUMENT;
    // ncclAllGather(sendbuff, recvbuff, sendcount, datatype, comm, stream); ncclFloat = 7 (rccl.h).  Resolved at run time so that
    // libdvo.so has no link-time dependency on a collective library it needs on multi-GPU hosts only.
    typedef int (*all_gather_fn)(const void*, void*, size_t, int, void*, hipStream_t);
    static all_gather_fn all_gather = nullptr;
    if (!all_gather) {
        void* h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (h) all_gather = reinterpret_cast<all_gather_fn>(dlsym(h, "ncclAllGather"));
        if (!all_gather) { set_error("librccl.so (ncclAllGather) could not be loaded"); return DVO_ERR_NOT_READY; }
    }
    if (b->mono ? b->mono->latest_id < 0 : !b->impl.have_poses) return DVO_ERR_NOT_READY;
    const float* src = b->mono ? b->mono->xi_world.as<float>() : b->impl.trk.xi_out.as<float>();   // (world twists / relative twists)
    DVO_TRY(select_device(b->device()));
    const int rc = all_gather(src, xi_all_dev, (size_t)b->n_seq() * 6, 7 /* ncclFloat */, rccl_comm, b->stream());
    if (rc != 0) { set_error("ncclAllGather failed"); return DVO_ERR_HIP; }
    return DVO_OK;
}

int dvo_batch_profile(dvo_batch* b, dvo_gn_profile* out, int reset)
{
    if (!b || !out) return DVO_ERR_BAD_ARGUMENT;
    Tracker& trk = b->trk();
    DVO_TRY(select_device(b->device()));
    DVO_TRY(trk.collect_profile(b->stream()));
    unsigned long long c[2] = {0, 0};
    DVO_HIP(hipMemcpy(c, trk.counters.p, sizeof c, hipMemcpyDeviceToHost));
    out->gn_ms = trk.prof_ms;
    out->gn_launches = trk.prof_launches;
    out->gn_pixels = c[0];
    out->gn_iterations = c[1];
    if (reset) {
        trk.prof_ms = 0; trk.prof_launches = 0;
        DVO_HIP(hipMemset(trk.counters.p, 0, sizeof c));
    }
    return DVO_OK;
}

int dvo_batch_probe_gn(dvo_batch* b, int level, int n_launches, float* avg_ms, uint64_t* pixels_per_launch)
{
    if (!b || !avg_ms || n_launches < 1) return DVO_ERR_BAD_ARGUMENT;
    DVO_NOT_MONO(b);
    Batch& B = b->impl;
    if (level < 0 || level >= B.g.levels) return DVO_ERR_BAD_ARGUMENT;
    if (B.cur < 0 || B.prev < 0 || !B.have_poses) return DVO_ERR_NOT_READY;
    DVO_TRY(select_device(B.device));
    // exactly the operands of the last track() call: obj = the newest frame set, ref = the one before it (keyframe tracking: obj = the
    // last frame's set, prev, and ref = the keyframe set, cur)
    const int obj = B.kf_on ? B.prev : B.cur, ref = B.kf_on ? B.cur : B.prev;
    const GnArgs ga = B.trk.gn_args(B.fs[obj], B.fs[ref], level, nullptr, 1);
    hipEvent_t e0, e1;
    DVO_HIP(hipEventCreate(&e0));
    DVO_HIP(hipEventCreate(&e1));
    B.trk.launch_gn(ga, level, B.trk.n_seq, B.stream);  // warm
    DVO_HIP(hipEventRecord(e0, B.stream));
    for (int i = 0; i < n_launches; i++) B.trk.launch_gn(ga, level, B.trk.n_seq, B.stream);
    DVO_HIP(hipEventRecord(e1, B.stream));
    DVO_HIP(hipEventSynchronize(e1));
    float ms = 0;
    DVO_HIP(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *avg_ms = ms / (float)n_launches;
    if (pixels_per_launch) *pixels_per_launch = (uint64_t)B.n_seq * B.g.w[level] * B.g.h[level];
    return DVO_OK;
}

// ------------------------------------------------------------------------------------------------ operator level
namespace {
struct OpCtx {  // device selection + a private stream for one operator call
    hipStream_t s = nullptr;
    int open(int dev)
    {
        DVO_TRY(select_device(dev));
        DVO_HIP(hipStreamCreate(&s));
        return DVO_OK;
    }
    ~OpCtx() { if (s) (void)hipStreamDestroy(s); }
};
int upload(DevBuf& b, const float* host, size_t count, hipStream_t s)
{
    DVO_TRY(b.alloc(count * sizeof(float)));
    DVO_HIP(hipMemcpyAsync(b.p, host, count * sizeof(float), hipMemcpyHostToDevice, s));
    return DVO_OK;
}
int download(float* host, const void* dev, size_t count, hipStream_t s)
{
    DVO_HIP(hipMemcpyAsync(host, dev, count * sizeof(float), hipMemcpyDeviceToHost, s));
    return DVO_OK;
}
Intr intr_of(const float K[9]) { return make_intr(K); }
}  // namespace

int dvo_op_cull_image(int dev, const float* src, int w, int h, int times, float* dst)
{
    if (!src || !dst || w < 1 || h < 1 || times < 0 || times > 8) return DVO_ERR_BAD_ARGUMENT;
    OpCtx c; DVO_TRY(c.open(dev));
    const size_t n = (size_t)w * h, dn = (size_t)(w >> times) * (h >> times);
    if (dn == 0) return DVO_OK;  // empty output, as cv::Mat::zeros(0 x 0)
    DevBuf a, b;
    DVO_TRY(upload(a, src, n, c.s));
    DVO_TRY(b.alloc(dn * 4));
    launch_cull(a.as<float>(), w, h, times, b.as<float>(), c.s);
    DVO_TRY(download(dst, b.p, dn, c.s));
    DVO_HIP(hipStreamSynchronize(c.s));
    return DVO_OK;
}

int dvo_op_gradient(int dev, const float* img, int w, int h, int xdir, float* out)
{
    if (!img || !out || w < 1 || h < 1) return DVO_ERR_BAD_ARGUMENT;
    OpCtx c; DVO_TRY(c.open(dev));
    const size_t n = (size_t)w * h;
    DevBuf a, b;
    DVO_TRY(upload(a, img, n, c.s));
    DVO_TRY(b.alloc(n * 4));
    launch_gradient(a.as<float>(), w, h, xdir, b.as<float>(), c.s);
    DVO_TRY(download(out, b.p, n, c.s));
    DVO_HIP(hipStreamSynchronize(c.s));
    return DVO_OK;
}

int dvo_op_warp_image(int dev, const float xi[6], const float* gray, const float* depth, int w, int h, const float K[9], float* out)
{
    if (!xi || !gray || !depth || !K || !out || w < 1 || h < 1) return DVO_ERR_BAD_ARGUMENT;
    OpCtx c; DVO_TRY(c.open(dev));
    const size_t n = (size_t)w * h;
    DevBuf g, d, o, xin, T;
    DVO_TRY(upload(g, gray, n, c.s));
    DVO_TRY(upload(d, depth, n, c.s));
    DVO_TRY(o.alloc(n * 4));
    // the pose comes from the DEVICE exp (that is what the tracker uses): exp(-xi)
    float neg[6];
    for (int i = 0; i < 6; i++) neg[i] = -xi[i];
    DVO_TRY(upload(xin, neg, 6, c.s));
    DVO_TRY(T.alloc(16 * 4));
    launch_se3(0, xin.as<float>(), nullptr, T.as<float>(), c.s);
    float Th[16];
    DVO_TRY(download(Th, T.p, 16, c.s));
    DVO_HIP(hipStreamSynchronize(c.s));
    Pose pose;
    for (int r = 0; r < 3; r++) {
        for (int q = 0; q < 3; q++) pose.R[3 * r + q] = Th[4 * r + q];
        pose.t[r] = Th[4 * r + 3];
    }
    launch_warp_image(g.as<float>(), d.as<float>(), w, h, intr_of(K), pose, o.as<float>(), c.s);
    DVO_TRY(download(out, o.p, n, c.s));
    DVO_HIP(hipStreamSynchronize(c.s));
    return DVO_OK;
}

int dvo_op_pyramid(int dev, const float* gray, const float* depth, const float* sigma, int w, int h, int levels, int culls,
                   float* const gray_out[], float* const depth_out[], float* const sigma_out[])
{
    if (!gray || !gray_out) return DVO_ERR_BAD_ARGUMENT;
    OpCtx c; DVO_TRY(c.open(dev));
    const float Kid[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    Geometry g;
    DVO_TRY(make_geometry(Kid, w, h, levels, culls, g));
    FrameSet fs;
    dvo_config dc;
    dvo_config_default(&dc);
    DVO_TRY(fs.alloc(g, 1, dc));
    const size_t n = (size_t)w * h;
    DevBuf a, b, s3;
    DVO_TRY(upload(a, gray, n, c.s));
    if (depth) DVO_TRY(upload(b, depth, n, c.s));
    if (sigma) DVO_TRY(upload(s3, sigma, n, c.s));
    build_pyramid(fs, a.as<float>(), depth ? b.as<float>() : nullptr, sigma ? s3.as<float>() : nullptr, c.s);
    for (int l = 0; l < levels; l++) {
        const size_t ln = (size_t)g.w[l] * g.h[l];
        if (gray_out[l]) DVO_TRY(download(gray_out[l], fs.gray[l], ln, c.s));
        if (depth && depth_out && depth_out[l]) DVO_TRY(download(depth_out[l], fs.depth[l], ln, c.s));
        if (sigma && sigma_out && sigma_out[l]) DVO_TRY(download(sigma_out[l], fs.sigma[l], ln, c.s));
    }
    DVO_HIP(hipStreamSynchronize(c.s));
    return DVO_OK;
}

namespace {
int bad_pyramid_frames(const char* what)
{
    set_error(std::string("dvo_op_pyramid_frames: ") + what);
    return DVO_ERR_BAD_ARGUMENT;
}
// one frame of every sequence of dvo_op_pyramid_frames on the device: `bytes` per image row times `rows` rows times n images each
struct OpFrames {
    DevBuf g, d, s;
    FrameInput in;
    int upload(const float* gray, const float* depth, const float* sigma, const uint8_t* rgb, int channels, const uint16_t* depth16,
               float depth_scale, size_t px, bool rows_decimated, hipStream_t st)
    {
        auto up = [&](DevBuf& b, const void* host, size_t bytes) -> int {
            DVO_TRY(b.alloc(bytes));
            DVO_HIP(hipMemcpyAsync(b.p, host, bytes, hipMemcpyHostToDevice, st));
            return DVO_OK;
        };
        in.rows_decimated = rows_decimated;
        if (rgb) {
            DVO_TRY(up(g, rgb, px * (size_t)channels));
            in.rgb = g.as<uint8_t>(); in.channels = channels; in.depth_scale = depth_scale;
            if (depth16) { DVO_TRY(up(d, depth16, px * sizeof(uint16_t))); in.depth16 = d.as<uint16_t>(); }
            return DVO_OK;
        }
        DVO_TRY(up(g, gray, px * sizeof(float)));
        in.gray = g.as<float>();
        if (depth) {
            DVO_TRY(up(d, depth, px * sizeof(float))); DVO_TRY(up(s, sigma, px * sizeof(float)));
            in.depth = d.as<float>(); in.sigma = s.as<float>();
        }
        return DVO_OK;
    }
};
}  // namespace

// dvo_op_pyramid_frames and, with a filter, dvo_op_pyramid_frames_filtered: the one body of both
static int pyramid_frames(int dev, const dvo_config* cfg, const dvo_pyramid_frames_args* args, int filter, float* const gray_out[],
                          float* const depth_out[], float* const sigma_out[], float* const wgt_out[], dvo_pyramid_kernel* ran)
{
    if (!args) return bad_pyramid_frames("args is NULL");
    if (args->struct_size != (int)sizeof(dvo_pyramid_frames_args)) return bad_pyramid_frames("struct_size is not sizeof(dvo_pyramid_frames_args)");
    const dvo_pyramid_frames_args& p = *args;
    if (p.n_seq < 1) return bad_pyramid_frames("n_seq < 1");
    const bool raw = p.rgb != nullptr;
    if (raw == (p.gray != nullptr)) return bad_pyramid_frames("exactly one of gray (float maps) and rgb (raw frames) must be given");
    if (raw && (p.depth || p.sigma || p.gray2 || p.depth2 || p.sigma2)) return bad_pyramid_frames("float maps beside raw frames");
    if (!raw && (p.depth16 || p.rgb2 || p.depth16_2)) return bad_pyramid_frames("raw frames beside float maps");
    if ((p.depth != nullptr) != (p.sigma != nullptr)) return bad_pyramid_frames("depth and sigma come together");
    if (raw && p.channels != 1 && p.channels != 3 && p.channels != 4) return bad_pyramid_frames("channels must be 1, 3 or 4");
    if (!std::isfinite(p.depth_scale) || p.depth_scale < 0.0f) return bad_pyramid_frames("depth_scale must be finite and >= 0");
    if (p.flags & ~(DVO_PYRAMID_ROWS_DECIMATED | DVO_PYRAMID_FORCE_WEIGHT_MAPS | DVO_PYRAMID_SPLIT)) return bad_pyramid_frames("unknown flag bits");
    if (filter != DVO_PYRAMID_FILTER_NONE) {
        if (filter != DVO_PYRAMID_FILTER_BINOMIAL3) return bad_pyramid_frames("filter is not DVO_PYRAMID_FILTER_NONE or DVO_PYRAMID_FILTER_BINOMIAL3");
        if (p.flags & (DVO_PYRAMID_ROWS_DECIMATED | DVO_PYRAMID_SPLIT)) return bad_pyramid_frames("a filtered build takes whole frames and is not split");
        if (p.culls > 2) return bad_pyramid_frames("the filtered build supports culls 0, 1 and 2");
    }
    const bool second = raw ? p.rgb2 != nullptr : p.gray2 != nullptr;
    if (p.seq_action) {
        if (!second) return bad_pyramid_frames("seq_action without second frames");
        if (raw ? (p.depth16_2 != nullptr) != (p.depth16 != nullptr)
                : ((p.depth2 != nullptr) != (p.depth != nullptr) || (p.sigma2 != nullptr) != (p.sigma != nullptr)))
            return bad_pyramid_frames("the second frames must carry the maps the first carry");
        for (int q = 0; q < p.n_seq; q++)
            if (p.seq_action[q] > DVO_SEQ_RESTART) return bad_pyramid_frames("an action is not DVO_SEQ_SKIP, DVO_SEQ_TRACK or DVO_SEQ_RESTART");
    } else if (second || p.depth2 || p.sigma2 || p.depth16_2) {
        return bad_pyramid_frames("second frames without seq_action");
    }
    const float Kid[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    Geometry g;
    DVO_TRY(make_geometry(Kid, p.w, p.h, p.levels, p.culls, g));
    const bool dec = (p.flags & DVO_PYRAMID_ROWS_DECIMATED) != 0;
    if (dec && !can_decimate_rows(g)) return bad_pyramid_frames("DVO_PYRAMID_ROWS_DECIMATED needs culls > 0 and a height that is a multiple of 2^culls");
    dvo_config dc;
    if (cfg) dc = *cfg; else dvo_config_default(&dc);

    OpCtx c; DVO_TRY(c.open(dev));
    const size_t px = (size_t)p.w * (size_t)(dec ? p.h >> p.culls : p.h) * (size_t)p.n_seq;
    const float scale = p.depth_scale > 0.0f ? p.depth_scale : 1.0f / 5000.0f;
    FrameSet A, B;
    OpFrames first, next;
    DevBuf act;
    DVO_TRY(A.alloc(g, p.n_seq, dc));
    DVO_HIP(hipMemsetAsync(A.arena.p, 0xff, A.arena.bytes, c.s));
    DVO_TRY(first.upload(p.gray, p.depth, p.sigma, p.rgb, p.channels, p.depth16, scale, px, dec, c.s));
    first.in.filter = next.in.filter = filter;
    if (p.flags & DVO_PYRAMID_FORCE_WEIGHT_MAPS) A.allow_const_weight = false;
    // the split build's second stream and events, as Batch owns them
    PyramidSplit split;
    struct SplitOwner {
        PyramidSplit& s;
        ~SplitOwner()
        {
            if (s.fork) (void)hipEventDestroy(s.fork);
            if (s.done) (void)hipEventDestroy(s.done);
            if (s.side) (void)hipStreamDestroy(s.side);
        }
    } owner{split};
    const bool want_split = (p.flags & DVO_PYRAMID_SPLIT) != 0;
    if (want_split) {
        DVO_HIP(hipStreamCreate(&split.side));
        DVO_HIP(hipEventCreateWithFlags(&split.fork, hipEventDisableTiming));
        DVO_HIP(hipEventCreateWithFlags(&split.done, hipEventDisableTiming));
    }
    PyramidKernel k;
    FrameSet* out = &A;
    if (!p.seq_action) {
        const bool halves = build_pyramid(A, first.in, c.s, /*keep_sigma=*/true, nullptr, nullptr, want_split ? &split : nullptr, &k);
        if (split.err != hipSuccess) DVO_HIP(split.err);
        if (halves) DVO_HIP(hipStreamWaitEvent(c.s, split.done, 0));
    } else {
        build_pyramid(A, first.in, c.s, /*keep_sigma=*/true);
        DVO_TRY(B.alloc(g, p.n_seq, dc));
        DVO_HIP(hipMemsetAsync(B.arena.p, 0xff, B.arena.bytes, c.s));
        if (p.flags & DVO_PYRAMID_FORCE_WEIGHT_MAPS) B.allow_const_weight = false;
        DVO_TRY(next.upload(p.gray2, p.depth2, p.sigma2, p.rgb2, p.channels, p.depth16_2, scale, px, dec, c.s));
        DVO_TRY(act.alloc(((size_t)p.n_seq + 15) & ~(size_t)15));
        DVO_HIP(hipMemcpyAsync(act.p, p.seq_action, (size_t)p.n_seq, hipMemcpyHostToDevice, c.s));
        const bool halves = build_pyramid(B, next.in, c.s, /*keep_sigma=*/true, act.as<uint8_t>(), &A, want_split ? &split : nullptr, &k);
        if (split.err != hipSuccess) DVO_HIP(split.err);
        if (halves) DVO_HIP(hipStreamWaitEvent(c.s, split.done, 0));
        out = &B;
    }
    for (int l = 0; l < g.levels; l++) {
        const size_t ln = (size_t)g.w[l] * g.h[l] * (size_t)p.n_seq;
        if (gray_out && gray_out[l]) DVO_TRY(download(gray_out[l], out->gray[l], ln, c.s));
        if (depth_out && depth_out[l]) DVO_TRY(download(depth_out[l], out->depth[l], ln, c.s));
        if (sigma_out && sigma_out[l]) DVO_TRY(download(sigma_out[l], out->sigma[l], ln, c.s));
        if (wgt_out && wgt_out[l]) DVO_TRY(download(wgt_out[l], out->wgt[l], ln, c.s));
    }
    DVO_HIP(hipStreamSynchronize(c.s));
    if (want_split) DVO_HIP(hipStreamSynchronize(split.side));
    if (ran) { ran->kind = k.kind; ran->culls = k.culls; ran->plan = k.plan; }
    return DVO_OK;
}

int dvo_op_pyramid_frames(int dev, const dvo_config* cfg, const dvo_pyramid_frames_args* args, float* const gray_out[],
                          float* const depth_out[], float* const sigma_out[], float* const wgt_out[], dvo_pyramid_kernel* ran)
{
    return pyramid_frames(dev, cfg, args, DVO_PYRAMID_FILTER_NONE, gray_out, depth_out, sigma_out, wgt_out, ran);
}

int dvo_op_pyramid_frames_filtered(int dev, const dvo_config* cfg, const dvo_pyramid_frames_args* args, int filter,
                                   float* const gray_out[], float* const depth_out[], float* const sigma_out[],
                                   float* const wgt_out[], dvo_pyramid_kernel* ran)
{
    return pyramid_frames(dev, cfg, args, filter, gray_out, depth_out, sigma_out, wgt_out, ran);
}

// The optional inputs and outputs of one evaluation, by term (value-initialised; each dvo_op_gn_step* fills what it uses):
//   rob: the weighted pair on the weighted plan with one entry of (kind, param, s2); with the median scale, the bin counts, the
//        median bin and the next entry's s2 come back through med_*
//   aff: the pair with one entry (a, b); the moments and the next entry come back
//   geo: the geometric pair -- ref_depth / ref_sigma are then the tracked frame's own maps and geo.ref_depth the reference's depth --
//        and its sums; with aff too, the combined pair
struct StepTerms {
    uint8_t* mask;
    struct { const dvo_robust_config* cfg; float s2; uint32_t* med_counts; int* med_bin; float* med_next_s2; } rob;
    struct { const dvo_affine_config* cfg; float a, b; double* moments; float* next_ab; } aff;
    struct { const dvo_geometric_config* cfg; const float* ref_depth; double* sums; } geo;
};

// dvo_op_gn_step and its per-term forms: one Gauss-Newton evaluation of one level at `xi`, through the launch pair a batch would run
static int gn_step(const char* who, int dev, const dvo_config* cfg, const float* obj_gray, const float* ref_gray, const float* ref_depth,
                   const float* ref_sigma, int w, int h, const float K[9], const float xi[6], int level, dvo_gn_result* out, const StepTerms& t)
{
    uint8_t* const mask = t.mask;
    if (!obj_gray || !ref_gray || !ref_depth || !ref_sigma || !K || !xi || !out || w < 1 || h < 1 || level < 0 || level >= DVO_MAX_LEVELS)
        return DVO_ERR_BAD_ARGUMENT;
    dvo_config cf;
    if (cfg) cf = *cfg; else dvo_config_default(&cf);
    OpCtx c; DVO_TRY(c.open(dev));
    // a one-level "pyramid" whose only level carries index `level` semantics (step size, crop)
    Geometry g;
    DVO_TRY(make_geometry(K, w, h, 1, 0, g));
    // place the level at index `level` so Tracker::level_params / logs see the right index
    Geometry gl = g;
    gl.levels = level + 1;
    for (int l = 0; l <= level; l++) { gl.w[l] = w; gl.h[l] = h; memcpy(gl.K9[l], g.K9[0], sizeof g.K9[0]); gl.k[l] = g.k[0]; }
    Tracker trk;
    DVO_TRY(trk.init(gl, 1, cf));
    if (t.rob.cfg) DVO_TRY(trk.set_robust(who, t.rob.cfg, c.s));
    if (t.geo.cfg && t.aff.cfg) DVO_TRY(trk.set_geometric_affine(who, t.geo.cfg, t.aff.cfg, c.s));
    else if (t.aff.cfg) DVO_TRY(trk.set_affine(who, t.aff.cfg, c.s));
    else if (t.geo.cfg) DVO_TRY(trk.set_geometric(who, t.geo.cfg, c.s));
    DevBuf mom, zr, zs, mn;   // the terms' device outputs, and the reference's depth
    if (trk.aff.on) DVO_TRY(mom.alloc(sizeof(double) * DVO_AFFINE_MOMENTS));
    if (trk.geo.on) {
        DVO_TRY(upload(zr, t.geo.ref_depth, (size_t)w * h, c.s));
        DVO_TRY(zs.alloc(sizeof(double) * 2));
    }
    if (trk.rob.median()) DVO_TRY(mn.alloc(sizeof(int) * 2));
    const size_t n = (size_t)w * h;
    DevBuf og, rg, rd, rs, mk, xin, res;
    DVO_TRY(upload(og, obj_gray, n, c.s));
    DVO_TRY(upload(rg, ref_gray, n, c.s));
    DVO_TRY(upload(rd, ref_depth, n, c.s));
    DVO_TRY(upload(rs, ref_sigma, n, c.s));
    DVO_TRY(upload(xin, xi, 6, c.s));
    DVO_TRY(res.alloc(sizeof(dvo_gn_result)));
    if (mask) { DVO_TRY(mk.alloc(n)); DVO_HIP(hipMemsetAsync(mk.p, 0, n, c.s)); }
    launch_set_pose(trk.state.as<SeqState>(), xin.as<float>(), 1, c.s);
    // per-pixel constants of the reference level (what build_pyramid does for whole frames)
    DevBuf wgb;
    DVO_TRY(wgb.alloc(n * 4));
    {
        PrepArgs pa{};
        pa.depth = rd.as<float>(); pa.sigma = rs.as<float>(); pa.wgt = wgb.as<float>();
        pa.level_end[0] = n;
        pa.step[0] = trk.level_params(level).step;
        pa.sigma_min = cf.sigma_min; pa.sigma_max = cf.sigma_max;
        pa.levels = 1;
        launch_prep_ref(pa, c.s);
    }
    const GnArgs ga = trk.gn_args(og.as<float>(), rg.as<float>(), rd.as<float>(), wgb.as<float>(), 0.0f, level, mask ? mk.as<uint8_t>() : nullptr, 1);
    const Tracker::GivenOnce once{t.rob.s2, t.aff.a, t.aff.b};
    DVO_TRY(trk.begin_terms(c.s, &once));
    trk.launch_gn_term(ga, level, 1, c.s, 0, zr.as<float>());
    SolveArgs sa = trk.solve_args(level, 0, 1, trk.pair_rows(level, SolveRows::Live));
    sa.log = nullptr;   // (one evaluation: the sums go to `res`, no iteration record)
    sa.result = res.as<dvo_gn_result>();
    Tracker::SolveTerm st{};
    st.estimate_once = true;
    st.geo_sums = zs.as<double>(); st.affine_moments = mom.as<double>(); st.step_mn = mn.as<int>();
    trk.launch_solve_term(sa, 1, c.s, st);
    int med_mn[2] = {0, 0};
    RobustEntry med_next{};
    if (trk.rob.median()) {
        DVO_HIP(hipMemcpyAsync(t.rob.med_counts, trk.rob.hist_last.p, sizeof(uint32_t) * DVO_MEDIAN_BINS, hipMemcpyDeviceToHost, c.s));
        DVO_HIP(hipMemcpyAsync(med_mn, mn.p, sizeof med_mn, hipMemcpyDeviceToHost, c.s));
        DVO_HIP(hipMemcpyAsync(&med_next, trk.rob.table.p, sizeof med_next, hipMemcpyDeviceToHost, c.s));
    }
    if (trk.aff.on) {
        DVO_HIP(hipMemcpyAsync(t.aff.moments, mom.p, sizeof(double) * DVO_AFFINE_MOMENTS, hipMemcpyDeviceToHost, c.s));
        DVO_HIP(hipMemcpyAsync(t.aff.next_ab, trk.aff.table.p, sizeof(float) * 2, hipMemcpyDeviceToHost, c.s));
    }
    if (trk.geo.on) DVO_HIP(hipMemcpyAsync(t.geo.sums, zs.p, sizeof(double) * 2, hipMemcpyDeviceToHost, c.s));
    DVO_HIP(hipMemcpyAsync(out, res.p, sizeof *out, hipMemcpyDeviceToHost, c.s));
    if (mask) DVO_HIP(hipMemcpyAsync(mask, mk.p, n, hipMemcpyDeviceToHost, c.s));
    DVO_HIP(hipStreamSynchronize(c.s));
    DVO_HIP(hipGetLastError());
    if (trk.rob.median()) { *t.rob.med_bin = med_mn[0]; *t.rob.med_next_s2 = med_next.s2; }
    return DVO_OK;
}

// kind NONE still runs the weighted pair of the robust operators, with the plain entry (rho = 1; an entry the solve writes is then
// Huber's with k = 1): the configuration and the s2 they hand to gn_step
static dvo_robust_config op_robust_config(int kind, float param, int scale_mode)
{
    dvo_robust_config rc{};
    rc.struct_size = (int)sizeof rc;
    rc.kind = kind == DVO_ROBUST_NONE ? DVO_ROBUST_HUBER : kind;
    rc.scale_mode = scale_mode;
    rc.param = kind == DVO_ROBUST_NONE ? 1.0f : param;
    return rc;   // (scale_floor 0, not validated here: GIVEN ignores it, the median scale then keeps the bin's own s2)
}

static dvo_geometric_config op_geometric_config(float weight, float max_diff)
{
    dvo_geometric_config gc{};
    gc.struct_size = (int)sizeof gc;
    gc.mode = DVO_GEOMETRIC_ON; gc.weight = weight; gc.max_diff = max_diff;
    return gc;
}

int dvo_op_gn_step_geometric(int dev, const dvo_config* cfg, const float* obj_gray, const float* obj_depth, const float* obj_sigma,
                             const float* ref_gray, const float* ref_depth, int w, int h, const float K[9], const float xi[6], int level,
                             float weight, float max_diff, dvo_gn_result* out, double sums[2])
{
    static const char who[] = "dvo_op_gn_step_geometric";
    if (!ref_depth || !sums) return DVO_ERR_BAD_ARGUMENT;
    const dvo_geometric_config gc = op_geometric_config(weight, max_diff);
    if (!geometric_config_ok(&gc, who)) return DVO_ERR_BAD_ARGUMENT;
    StepTerms t{};
    t.geo = {&gc, ref_depth, sums};
    return gn_step(who, dev, cfg, obj_gray, ref_gray, obj_depth, obj_sigma, w, h, K, xi, level, out, t);
}

int dvo_op_gn_step_geometric_affine(int dev, const dvo_config* cfg, const float* obj_gray, const float* obj_depth, const float* obj_sigma,
                                    const float* ref_gray, const float* ref_depth, int w, int h, const float K[9], const float xi[6],
                                    int level, float weight, float max_diff, float a, float b, dvo_gn_result* out, double sums[2],
                                    double moments[5], float next_ab[2])
{
    static const char who[] = "dvo_op_gn_step_geometric_affine";
    if (!ref_depth || !sums || !moments || !next_ab) return DVO_ERR_BAD_ARGUMENT;
    const dvo_geometric_config gc = op_geometric_config(weight, max_diff);
    if (!geometric_config_ok(&gc, who)) return DVO_ERR_BAD_ARGUMENT;
    const dvo_affine_config ac = affine_config_given();
    StepTerms t{};
    t.geo = {&gc, ref_depth, sums};
    t.aff = {&ac, a, b, moments, next_ab};
    return gn_step(who, dev, cfg, obj_gray, ref_gray, obj_depth, obj_sigma, w, h, K, xi, level, out, t);
}

int dvo_op_gn_step(int dev, const dvo_config* cfg, const float* obj_gray, const float* ref_gray, const float* ref_depth,
                   const float* ref_sigma, int w, int h, const float K[9], const float xi[6], int level,
                   dvo_gn_result* out, uint8_t* mask)
{
    StepTerms t{};
    t.mask = mask;
    return gn_step("dvo_op_gn_step", dev, cfg, obj_gray, ref_gray, ref_depth, ref_sigma, w, h, K, xi, level, out, t);
}

int dvo_op_gn_step_robust(int dev, const dvo_config* cfg, const float* obj_gray, const float* ref_gray, const float* ref_depth,
                          const float* ref_sigma, int w, int h, const float K[9], const float xi[6], int level,
                          int kind, float param, float s2, dvo_gn_result* out)
{
    static const char who[] = "dvo_op_gn_step_robust";
    if (!robust_kind_param_ok(who, kind, param)) return DVO_ERR_BAD_ARGUMENT;
    const dvo_robust_config rc = op_robust_config(kind, param, DVO_ROBUST_SCALE_GIVEN);
    StepTerms t{};
    t.rob.cfg = &rc; t.rob.s2 = kind == DVO_ROBUST_NONE ? 0.0f : s2;
    return gn_step(who, dev, cfg, obj_gray, ref_gray, ref_depth, ref_sigma, w, h, K, xi, level, out, t);
}

int dvo_op_gn_step_robust_median(int dev, const dvo_config* cfg, const float* obj_gray, const float* ref_gray, const float* ref_depth,
                                 const float* ref_sigma, int w, int h, const float K[9], const float xi[6], int level,
                                 int kind, float param, float s2, dvo_gn_result* out, uint32_t counts[256], int* median_bin, float* next_s2)
{
    static const char who[] = "dvo_op_gn_step_robust_median";
    if (!counts || !median_bin || !next_s2) return DVO_ERR_BAD_ARGUMENT;
    if (!robust_kind_param_ok(who, kind, param)) return DVO_ERR_BAD_ARGUMENT;
    const dvo_robust_config rc = op_robust_config(kind, param, DVO_ROBUST_SCALE_MEDIAN);
    StepTerms t{};
    t.rob = {&rc, kind == DVO_ROBUST_NONE ? 0.0f : s2, counts, median_bin, next_s2};
    return gn_step(who, dev, cfg, obj_gray, ref_gray, ref_depth, ref_sigma, w, h, K, xi, level, out, t);
}

int dvo_op_gn_step_affine(int dev, const dvo_config* cfg, const float* obj_gray, const float* ref_gray, const float* ref_depth,
                          const float* ref_sigma, int w, int h, const float K[9], const float xi[6], int level,
                          int kind, float param, float s2, float a, float b, dvo_gn_result* out, double moments[5], float next_ab[2])
{
    static const char who[] = "dvo_op_gn_step_affine";
    if (!moments || !next_ab) return DVO_ERR_BAD_ARGUMENT;
    if (!robust_kind_param_ok(who, kind, param)) return DVO_ERR_BAD_ARGUMENT;
    const dvo_robust_config rc = op_robust_config(kind, param, DVO_ROBUST_SCALE_GIVEN);
    const dvo_affine_config ac = affine_config_given();
    StepTerms t{};
    if (kind != DVO_ROBUST_NONE) { t.rob.cfg = &rc; t.rob.s2 = s2; }   // (kind NONE runs the instance without robust weights: rho = 1, N = n_valid)
    t.aff = {&ac, a, b, moments, next_ab};
    return gn_step(who, dev, cfg, obj_gray, ref_gray, ref_depth, ref_sigma, w, h, K, xi, level, out, t);
}

int dvo_op_track(int dev, const dvo_config* cfg, const float* obj_gray, const float* ref_gray, const float* ref_depth,
                 const float* ref_sigma, int w, int h, const float K[9], int levels, int culls, float xi_out[6], dvo_track_log* log)
{
    if (!obj_gray || !ref_gray || !ref_depth || !ref_sigma || !K || !xi_out) return DVO_ERR_BAD_ARGUMENT;
    dvo_config cf;
    if (cfg) cf = *cfg; else dvo_config_default(&cf);
    OpCtx c; DVO_TRY(c.open(dev));
    Geometry g;
    DVO_TRY(make_geometry(K, w, h, levels, culls, g));
    FrameSet obj, ref;
    DVO_TRY(obj.alloc(g, 1, cf));
    DVO_TRY(ref.alloc(g, 1, cf));
    Tracker trk;
    DVO_TRY(trk.init(g, 1, cf));
    const size_t n = (size_t)w * h;
    DevBuf og, rg, rd, rs;
    DVO_TRY(upload(og, obj_gray, n, c.s));
    DVO_TRY(upload(rg, ref_gray, n, c.s));
    DVO_TRY(upload(rd, ref_depth, n, c.s));
    DVO_TRY(upload(rs, ref_sigma, n, c.s));
    build_pyramid(obj, og.as<float>(), nullptr, nullptr, c.s);
    build_pyramid(ref, rg.as<float>(), rd.as<float>(), rs.as<float>(), c.s);
    DVO_TRY(trk.track(obj, ref, c.s));
    DVO_TRY(download(xi_out, trk.xi_out.p, 6, c.s));
    if (log) DVO_HIP(hipMemcpyAsync(log, trk.log.p, sizeof *log, hipMemcpyDeviceToHost, c.s));
    DVO_HIP(hipStreamSynchronize(c.s));
    return DVO_OK;
}

int dvo_op_propagate(int dev, const float* ref_depth, const float* ref_sigma, const float* ref_age, int w, int h,
                     const float xi[6], const float K[9], float* depth, float* sigma, float* age)
{
    if (!ref_depth || !ref_sigma || !ref_age || !xi || !K || !depth || !sigma || !age || w < 1 || h < 1) return DVO_ERR_BAD_ARGUMENT;
    OpCtx c; DVO_TRY(c.open(dev));
    const size_t n = (size_t)w * h;
    DevBuf a, b, g, od, os, oa, ow;
    DVO_TRY(upload(a, ref_depth, n, c.s));
    DVO_TRY(upload(b, ref_sigma, n, c.s));
    DVO_TRY(upload(g, ref_age, n, c.s));
    DVO_TRY(od.alloc(n * 4)); DVO_TRY(os.alloc(n * 4)); DVO_TRY(oa.alloc(n * 4)); DVO_TRY(ow.alloc(n * 4));
    Pose pose;
    pose_from_xi(xi, 1.0f, pose);  // host double exp, as VisualOdometry::map_propagate does
    launch_propagate(a.as<float>(), b.as<float>(), g.as<float>(), w, h, intr_of(K), pose, xi[2], ow.as<int>(),
                     od.as<float>(), os.as<float>(), oa.as<float>(), c.s);
    DVO_TRY(download(depth, od.p, n, c.s));
    DVO_TRY(download(sigma, os.p, n, c.s));
    DVO_TRY(download(age, oa.p, n, c.s));
    DVO_HIP(hipStreamSynchronize(c.s));
    return DVO_OK;
}

int dvo_op_regularize(int dev, const float* depth, const float* sigma, int w, int h, float* out)
{
    if (!depth || !sigma || !out || w < 1 || h < 1) return DVO_ERR_BAD_ARGUMENT;
    OpCtx c; DVO_TRY(c.open(dev));
    const size_t n = (size_t)w * h;
    DevBuf a, b, o;
    DVO_TRY(upload(a, depth, n, c.s));
    DVO_TRY(upload(b, sigma, n, c.s));
    DVO_TRY(o.alloc(n * 4));
    launch_regularize(a.as<float>(), b.as<float>(), w, h, o.as<float>(), c.s);
    DVO_TRY(download(out, o.p, n, c.s));
    DVO_HIP(hipStreamSynchronize(c.s));
    return DVO_OK;
}

int dvo_op_depth_update(int dev, const dvo_config* cfg, int n_hist, const float* const hist_gray[], const float* hist_xi,
                        const float* obj_gray, const float obj_xi[6], const float obj_rel_xi[6], int obj_id,
                        const float K[9], int w, int h, float* ref_depth, float* ref_sigma, float* ref_age, int* valid_updates)
{
    if (n_hist < 1 || !hist_gray || !hist_xi || !obj_gray || !obj_xi || !obj_rel_xi || !K || !ref_depth || !ref_sigma || !ref_age)
        return DVO_ERR_BAD_ARGUMENT;
    dvo_config cf;
    if (cfg) cf = *cfg; else dvo_config_default(&cf);
    OpCtx c; DVO_TRY(c.open(dev));
    const size_t n = (size_t)w * h;
    std::vector<DevBuf> grays(n_hist);
    std::vector<AgeEntry> tab(n_hist);
    std::vector<const float*> gptr(n_hist);
    for (int i = 0; i < n_hist; i++) {
        DVO_TRY(upload(grays[i], hist_gray[i], n, c.s));
        float nb[6], r_xi[6];
        for (int k = 0; k < 6; k++) nb[k] = -hist_xi[6 * i + k];
        se3_concatenate_f(obj_xi, nb, r_xi);
        pose_from_xi(r_xi, -1.0f, tab[i].pose);
        for (int k = 0; k < 3; k++) tab[i].tneg[k] = -r_xi[k];
        tab[i].slot = i;
        gptr[i] = grays[i].as<float>();
    }
    DevBuf og, rd, rs, ra, ages, vd, gtab;
    DVO_TRY(upload(og, obj_gray, n, c.s));
    DVO_TRY(upload(rd, ref_depth, n, c.s));
    DVO_TRY(upload(rs, ref_sigma, n, c.s));
    DVO_TRY(upload(ra, ref_age, n, c.s));
    DVO_TRY(ages.alloc(sizeof(AgeEntry) * (size_t)n_hist));
    DVO_HIP(hipMemcpyAsync(ages.p, tab.data(), sizeof(AgeEntry) * (size_t)n_hist, hipMemcpyHostToDevice, c.s));
    DVO_TRY(gtab.alloc(sizeof(float*) * (size_t)n_hist));
    DVO_HIP(hipMemcpyAsync(gtab.p, gptr.data(), sizeof(float*) * (size_t)n_hist, hipMemcpyHostToDevice, c.s));
    DVO_TRY(vd.alloc(sizeof(int)));
    DVO_HIP(hipMemsetAsync(vd.p, 0, sizeof(int), c.s));
    UpdateArgs a{};
    a.ref_depth = rd.as<float>(); a.ref_sigma = rs.as<float>(); a.ref_age = ra.as<float>();
    a.obj_gray = og.as<float>(); a.ages = ages.as<AgeEntry>(); a.gray_table = gtab.as<const float*>();
    a.n_seq = 1; a.R = n_hist;
    a.n_hist = n_hist; a.w = w; a.h = h; a.crop = cf.crop_enable; a.obj_id = obj_id; a.seed = cf.rng_seed;
    a.k = intr_of(K);
    memcpy(a.K9, K, sizeof a.K9);
    pose_from_xi(obj_rel_xi, 1.0f, a.rel_pose);
    a.rel_tz = obj_rel_xi[2];
    a.valid_updates = vd.as<int>();
    launch_depth_update(a, c.s);
    DVO_TRY(download(ref_depth, rd.p, n, c.s));
    DVO_TRY(download(ref_sigma, rs.p, n, c.s));
    DVO_TRY(download(ref_age, ra.p, n, c.s));
    int v = 0;
    DVO_HIP(hipMemcpyAsync(&v, vd.p, sizeof v, hipMemcpyDeviceToHost, c.s));
    DVO_HIP(hipStreamSynchronize(c.s));
    if (valid_updates) *valid_updates = v;
    return DVO_OK;
}

namespace {
int bad_update_batch(const char* what)
{
    set_error(std::string("dvo_op_depth_update_batch: ") + what);
    return DVO_ERR_BAD_ARGUMENT;
}
}  // namespace

int dvo_op_depth_update_batch(int dev, const dvo_config* cfg, const dvo_depth_update_batch_args* args, float* depth, float* sigma,
                              float* age, int* valid_updates, int* clamped)
{
    if (!args) return bad_update_batch("args is NULL");
    if (args->struct_size != (int)sizeof(dvo_depth_update_batch_args)) return bad_update_batch("struct_size is not sizeof(dvo_depth_update_batch_args)");
    const dvo_depth_update_batch_args& p = *args;
    if (p.n_seq < 1) return bad_update_batch("n_seq < 1");
    if (!p.K || !p.n_total || !p.kf_gray || !p.kf_xi || !p.obj_gray || !p.obj_xi || !p.obj_rel_xi || !p.need || !p.frame_id)
        return bad_update_batch("a NULL input");
    if (!depth || !sigma || !age) return bad_update_batch("a NULL map");
    if (p.w < 64 || p.h < 64) return bad_update_batch("w or h < 64");
    if (p.ring < 1 || p.ring > 64) return bad_update_batch("ring outside 1 .. 64");
    DVO_TRY(check_intrinsics("dvo_op_depth_update_batch", p.K, p.per_camera ? (size_t)p.n_seq : 1));
    for (int q = 0; q < p.n_seq; q++) {
        if (p.n_total[q] < 1) return bad_update_batch("n_total < 1");
        if (p.need[q] != 0 && p.need[q] != 1) return bad_update_batch("need is not 0 or 1");
    }
    dvo_config dc;
    if (cfg) dc = *cfg; else dvo_config_default(&dc);
    dc.device = dev;
    dc.stream = nullptr;
    MonoBatch mb;
    DVO_TRY(mb.init(p.n_seq, p.K, p.w, p.h, p.ring, &dc, p.per_camera != 0));
    const int T = mb.g.top(), R = p.ring;
    const size_t np = (size_t)mb.top_pixels(), ns = (size_t)p.n_seq;
    hipStream_t st = mb.stream;
    // the sequences' state as k_mono_decide / k_mono_commit leave it: the ring by slot, the frame's poses, the flags
    std::vector<MonoSeq> meta(ns);
    std::vector<float> hx(ns * R * 6, 0.0f);
    memset(meta.data(), 0, sizeof(MonoSeq) * ns);
    DVO_HIP(hipMemsetAsync(mb.ring_gray.p, 0xff, mb.ring_gray.bytes, st));   // (a slot no keyframe was given for: NaN)
    for (size_t q = 0; q < ns; q++) {
        MonoSeq& m = meta[q];
        const int n_total = p.n_total[q], n_hist = n_total < R ? n_total : R;
        for (int i = 0; i < n_hist; i++) {
            const int slot = (n_total - n_hist + i) % R;
            memcpy(&hx[(q * R + slot) * 6], p.kf_xi + (q * R + i) * 6, 6 * sizeof(float));
            DVO_HIP(hipMemcpyAsync(mb.ring_gray.as<float>() + (q * R + slot) * np, p.kf_gray + (q * R + i) * np, np * sizeof(float),
                                   hipMemcpyHostToDevice, st));
        }
        for (int k = 0; k < 6; k++) {
            m.ref_xi[k] = p.kf_xi[(q * R + (n_hist - 1)) * 6 + k];
            m.frame_xi[k] = p.obj_xi[q * 6 + k];
            m.rel_xi[k] = p.obj_rel_xi[q * 6 + k];
        }
        pose_from_xi(m.rel_xi, 1.0f, m.rel_pose);
        m.n_total = n_total; m.frame_id = p.frame_id[q]; m.need = p.need[q];
    }
    DVO_HIP(hipMemcpyAsync(mb.meta.p, meta.data(), sizeof(MonoSeq) * ns, hipMemcpyHostToDevice, st));
    DVO_HIP(hipMemcpyAsync(mb.hist_xi.p, hx.data(), hx.size() * sizeof(float), hipMemcpyHostToDevice, st));
    DVO_HIP(hipMemcpyAsync(mb.ref.depth[T], depth, ns * np * sizeof(float), hipMemcpyHostToDevice, st));
    DVO_HIP(hipMemcpyAsync(mb.ref.sigma[T], sigma, ns * np * sizeof(float), hipMemcpyHostToDevice, st));
    DVO_HIP(hipMemcpyAsync(mb.ref_age.p, age, ns * np * sizeof(float), hipMemcpyHostToDevice, st));
    DVO_HIP(hipMemcpyAsync(mb.frm.gray[T], p.obj_gray, ns * np * sizeof(float), hipMemcpyHostToDevice, st));
    DVO_TRY(mb.queue_depth_update(0, nullptr));   // (every sequence reads its own MonoSeq::frame_id)
    DVO_HIP(hipGetLastError());
    DVO_TRY(download(depth, mb.ref.depth[T], ns * np, st));
    DVO_TRY(download(sigma, mb.ref.sigma[T], ns * np, st));
    DVO_TRY(download(age, mb.ref_age.p, ns * np, st));
    DVO_HIP(hipMemcpyAsync(meta.data(), mb.meta.p, sizeof(MonoSeq) * ns, hipMemcpyDeviceToHost, st));
    DVO_HIP(hipStreamSynchronize(st));
    for (size_t q = 0; q < ns; q++) {
        if (valid_updates) valid_updates[q] = meta[q].valid_updates;
        if (clamped) clamped[q] = meta[q].clamped;
    }
    return DVO_OK;
}

int dvo_op_ingest(int dev, const uint8_t* rgb, int channels, const uint16_t* depth16, int w, int h, float depth_scale,
                  float sigma_valid, float sigma_invalid, int invalidate_gray, float* gray, float* depth, float* sigma)
{
    if (!rgb || !gray || w < 1 || h < 1 || (channels != 1 && channels != 3 && channels != 4)) return DVO_ERR_BAD_ARGUMENT;
    if (depth16 && (!depth || !sigma)) return DVO_ERR_BAD_ARGUMENT;
    OpCtx c; DVO_TRY(c.open(dev));
    const size_t n = (size_t)w * h;
    DevBuf r, d16, g, d, s;
    DVO_TRY(r.alloc(n * channels));
    DVO_HIP(hipMemcpyAsync(r.p, rgb, n * channels, hipMemcpyHostToDevice, c.s));
    if (depth16) {
        DVO_TRY(d16.alloc(n * 2));
        DVO_HIP(hipMemcpyAsync(d16.p, depth16, n * 2, hipMemcpyHostToDevice, c.s));
        DVO_TRY(d.alloc(n * 4)); DVO_TRY(s.alloc(n * 4));
    }
    DVO_TRY(g.alloc(n * 4));
    launch_ingest(r.as<uint8_t>(), channels, depth16 ? d16.as<uint16_t>() : nullptr, (int)n, depth_scale, sigma_valid, sigma_invalid,
                  invalidate_gray, g.as<float>(), d.as<float>(), s.as<float>(), c.s);
    DVO_TRY(download(gray, g.p, n, c.s));
    if (depth16) { DVO_TRY(download(depth, d.p, n, c.s)); DVO_TRY(download(sigma, s.p, n, c.s)); }
    DVO_HIP(hipStreamSynchronize(c.s));
    return DVO_OK;
}

int dvo_op_visualize(int dev, int mode, const float* a, const float* b, int w, int h, uint8_t* rgb)
{
    if (!a || !rgb || w < 1 || h < 1 || mode < 0 || mode > 4) return DVO_ERR_BAD_ARGUMENT;
    OpCtx c; DVO_TRY(c.open(dev));
    const size_t n = (size_t)w * h;
    DevBuf da, db, out;
    DVO_TRY(upload(da, a, n, c.s));
    if (b) DVO_TRY(upload(db, b, n, c.s));
    DVO_TRY(out.alloc(n * 3));
    launch_visualize(mode, da.as<float>(), b ? db.as<float>() : nullptr, (int)n, out.as<uint8_t>(), c.s);
    DVO_HIP(hipMemcpyAsync(rgb, out.p, n * 3, hipMemcpyDeviceToHost, c.s));
    DVO_HIP(hipStreamSynchronize(c.s));
    return DVO_OK;
}

int dvo_op_undistort(int dev, const float* src, int w, int h, const float K[9], const float D[5], float* dst)
{
    if (!src || !dst || !K || !D || w < 1 || h < 1) return DVO_ERR_BAD_ARGUMENT;
    OpCtx c; DVO_TRY(c.open(dev));
    const size_t n = (size_t)w * h;
    DevBuf a, b;
    DVO_TRY(upload(a, src, n, c.s));
    DVO_TRY(b.alloc(n * 4));
    launch_undistort(a.as<float>(), w, h, intr_of(K), D, DVO_INVALID, b.as<float>(), c.s);
    DVO_TRY(download(dst, b.p, n, c.s));
    DVO_HIP(hipStreamSynchronize(c.s));
    return DVO_OK;
}

static int se3_op(int dev, int op, const float* a, int na, const float* b, float* out, int nout)
{
    OpCtx c; DVO_TRY(c.open(dev));
    DevBuf da, db, dout;
    DVO_TRY(upload(da, a, na, c.s));
    if (b) DVO_TRY(upload(db, b, 6, c.s));
    DVO_TRY(dout.alloc(16 * 4));
    launch_se3(op, da.as<float>(), b ? db.as<float>() : nullptr, dout.as<float>(), c.s);
    DVO_TRY(download(out, dout.p, nout, c.s));
    DVO_HIP(hipStreamSynchronize(c.s));
    return DVO_OK;
}

int dvo_op_se3_exp(int dev, const float xi[6], float T[16]) { return (xi && T) ? se3_op(dev, 0, xi, 6, nullptr, T, 16) : DVO_ERR_BAD_ARGUMENT; }
int dvo_op_se3_log(int dev, const float T[16], float xi[6]) { return (xi && T) ? se3_op(dev, 1, T, 16, nullptr, xi, 6) : DVO_ERR_BAD_ARGUMENT; }
int dvo_op_se3_concatenate(int dev, const float a[6], const float b[6], float out[6])
{
    return (a && b && out) ? se3_op(dev, 2, a, 6, b, out, 6) : DVO_ERR_BAD_ARGUMENT;
}

int dvo_op_pose_algebra(int dev, int op, int n, const double* in, double* out)
{
    int ni, no;
    if (!in || !out || n < 1 || !pose_algebra_row(op, ni, no)) return DVO_ERR_BAD_ARGUMENT;
    OpCtx c; DVO_TRY(c.open(dev));
    DevBuf din, dout;
    const size_t bi = (size_t)n * ni * sizeof(double), bo = (size_t)n * no * sizeof(double);
    DVO_TRY(din.alloc(bi));
    DVO_TRY(dout.alloc(bo));
    DVO_HIP(hipMemcpyAsync(din.p, in, bi, hipMemcpyHostToDevice, c.s));
    launch_pose_algebra(op, n, din.as<double>(), dout.as<double>(), c.s);
    DVO_HIP(hipMemcpyAsync(out, dout.p, bo, hipMemcpyDeviceToHost, c.s));
    DVO_HIP(hipStreamSynchronize(c.s));
    return DVO_OK;
}

int dvo_op_lm_step(int dev, int n, const double* sums, const float* xi_eval, const dvo_lm_entry* entry_in, const dvo_lm_config* cfg,
                   int level_first, int it_prev, int max_iterations, int fixed_iterations, float min_update, float min_residual,
                   dvo_lm_entry* entry_out, float* update, float* xi_next, int* decision, int* active)
{
    if (!sums || !xi_eval || !entry_in || !cfg || !entry_out || !update || !xi_next || !decision || !active || n < 1) return DVO_ERR_BAD_ARGUMENT;
    if (!lm_config_ok(cfg, "dvo_op_lm_step")) return DVO_ERR_BAD_ARGUMENT;
    if (cfg->mode != DVO_LM_ON) { set_error("dvo_op_lm_step: the mode must be DVO_LM_ON"); return DVO_ERR_BAD_ARGUMENT; }
    OpCtx c; DVO_TRY(c.open(dev));
    const size_t N = (size_t)n;
    DevBuf dsums, dxi, table, state, last, upd, dec;
    DVO_TRY(dsums.alloc(N * 29 * sizeof(double)));
    DVO_TRY(dxi.alloc(N * 6 * sizeof(float)));
    DVO_TRY(table.alloc(N * sizeof(dvo_lm_entry)));
    DVO_TRY(state.alloc(N * sizeof(SeqState)));
    DVO_TRY(last.alloc(N * sizeof(dvo_lm_record)));
    DVO_TRY(upd.alloc(N * 6 * sizeof(float)));
    DVO_TRY(dec.alloc(N * sizeof(int)));
    DVO_HIP(hipMemcpyAsync(dsums.p, sums, dsums.bytes, hipMemcpyHostToDevice, c.s));
    DVO_HIP(hipMemcpyAsync(dxi.p, xi_eval, dxi.bytes, hipMemcpyHostToDevice, c.s));
    DVO_HIP(hipMemcpyAsync(table.p, entry_in, table.bytes, hipMemcpyHostToDevice, c.s));
    DVO_HIP(hipMemsetAsync(state.p, 0, state.bytes, c.s));
    DVO_HIP(hipMemsetAsync(last.p, 0, last.bytes, c.s));
    SolveArgs sa{};
    sa.state = state.as<SeqState>();
    sa.level = 0;
    sa.max_iterations = max_iterations; sa.fixed_iterations = fixed_iterations;
    sa.min_update = min_update; sa.min_residual = min_residual;
    sa.ignore_active = level_first ? 1 : 0;
    sa.n_seq = n;
    LmSolve m{};
    m.table = table.as<dvo_lm_entry>(); m.last = last.as<dvo_lm_record>();
    m.upd_out = upd.as<float>(); m.decision_out = dec.as<int>();
    m.levels = 1; m.log_its = 0;
    m.lambda_up = cfg->lambda_up; m.lambda_down = cfg->lambda_down; m.lambda_floor = cfg->lambda_floor;
    m.lambda_max = cfg->lambda_max; m.min_valid_fraction = cfg->min_valid_fraction;
    launch_lm_step(sa, m, dsums.as<double>(), dxi.as<float>(), n, it_prev, c.s);
    DVO_HIP(hipGetLastError());
    std::vector<SeqState> hs(N);
    DVO_HIP(hipMemcpyAsync(entry_out, table.p, table.bytes, hipMemcpyDeviceToHost, c.s));
    DVO_HIP(hipMemcpyAsync(update, upd.p, upd.bytes, hipMemcpyDeviceToHost, c.s));
    DVO_HIP(hipMemcpyAsync(decision, dec.p, dec.bytes, hipMemcpyDeviceToHost, c.s));
    DVO_HIP(hipMemcpyAsync(hs.data(), state.p, state.bytes, hipMemcpyDeviceToHost, c.s));
    DVO_HIP(hipStreamSynchronize(c.s));
    for (size_t i = 0; i < N; i++) {
        memcpy(xi_next + 6 * i, hs[i].xi, sizeof(float) * 6);
        active[i] = hs[i].active;
    }
    return DVO_OK;
}

int dvo_selftest_reciprocal(int dev, uint64_t* fast_path_inputs, uint64_t* mismatches, uint32_t* first_bad_bits)
{
    if (!mismatches) return DVO_ERR_BAD_ARGUMENT;
    DVO_TRY(select_device(dev));
    DevBuf out;
    DVO_TRY(out.alloc(3 * sizeof(unsigned long long)));
    unsigned long long h[3] = {0ull, 0ull, ~0ull};
    DVO_HIP(hipMemcpy(out.p, h, sizeof h, hipMemcpyHostToDevice));
    launch_selftest_reciprocal(out.as<unsigned long long>(), nullptr);
    DVO_HIP(hipDeviceSynchronize());
    DVO_HIP(hipMemcpy(h, out.p, sizeof h, hipMemcpyDeviceToHost));
    if (fast_path_inputs) *fast_path_inputs = h[0];
    *mismatches = h[1];
    if (first_bad_bits) *first_bad_bits = (uint32_t)h[2];
    return DVO_OK;
}

int dvo_selftest_trig(int dev, double* max_rel_sin, double* max_rel_cos, double* max_rel_atan2, uint64_t* samples)
{
    if (!max_rel_sin || !max_rel_cos || !max_rel_atan2) return DVO_ERR_BAD_ARGUMENT;
    DVO_TRY(select_device(dev));
    DevBuf out;
    DVO_TRY(out.alloc(3 * sizeof(unsigned long long)));
    DVO_HIP(hipMemset(out.p, 0, out.bytes));
    const unsigned side = 4096, n = side * side;
    launch_selftest_trig(n, side, out.as<unsigned long long>(), nullptr);
    DVO_HIP(hipDeviceSynchronize());
    unsigned long long h[3];
    DVO_HIP(hipMemcpy(h, out.p, sizeof h, hipMemcpyDeviceToHost));
    memcpy(max_rel_sin, &h[0], 8); memcpy(max_rel_cos, &h[1], 8); memcpy(max_rel_atan2, &h[2], 8);
    if (samples) *samples = n;
    return DVO_OK;
}

int dvo_selftest_sqrt(int dev, uint64_t* inputs, uint64_t* mismatches, uint32_t* first_bad_bits)
{
    if (!mismatches) return DVO_ERR_BAD_ARGUMENT;
    DVO_TRY(select_device(dev));
    DevBuf out;
    DVO_TRY(out.alloc(3 * sizeof(unsigned long long)));
    unsigned long long h[3] = {0ull, 0ull, ~0ull};
    DVO_HIP(hipMemcpy(out.p, h, sizeof h, hipMemcpyHostToDevice));
    launch_selftest_sqrt(out.as<unsigned long long>(), nullptr);
    DVO_HIP(hipDeviceSynchronize());
    DVO_HIP(hipMemcpy(h, out.p, sizeof h, hipMemcpyDeviceToHost));
    if (inputs) *inputs = h[0];
    *mismatches = h[1];
    if (first_bad_bits) *first_bad_bits = (uint32_t)h[2];
    return DVO_OK;
}

int dvo_selftest_division(int dev, uint32_t b_first, uint32_t b_stride, uint32_t b_count, uint64_t* pairs, uint64_t* mismatches, uint64_t* first_bad_pair)
{
    if (!mismatches || b_count == 0 || b_count > (1u << 23)) return DVO_ERR_BAD_ARGUMENT;
    DVO_TRY(select_device(dev));
    DevBuf out;
    DVO_TRY(out.alloc(3 * sizeof(unsigned long long)));
    unsigned long long h[3] = {0ull, 0ull, ~0ull};
    DVO_HIP(hipMemcpy(out.p, h, sizeof h, hipMemcpyHostToDevice));
    for (uint32_t done = 0; done < b_count; done += 1u << 17) {   // 2^17 values of b (x 2^23 of a) per launch: each well under a second
        const uint32_t n = b_count - done < (1u << 17) ? b_count - done : (1u << 17);
        launch_selftest_division(b_first + done * b_stride, b_stride, n, out.as<unsigned long long>(), nullptr);
        DVO_HIP(hipDeviceSynchronize());
    }
    DVO_HIP(hipMemcpy(h, out.p, sizeof h, hipMemcpyDeviceToHost));
    if (pairs) *pairs = h[0];
    *mismatches = h[1];
    if (first_bad_pair) *first_bad_pair = h[2];
    return DVO_OK;
}

}  // extern "C"
