// coeb_capi.hip -- context and the C-ABI of include/coeb_front.h.
//
// Host work here is the per-call argument marshalling, plus the geometry plan of coeb_plan.cpp
// once per image size (cached).  All per-pixel / per-keypoint work runs in the kernels of
// coeb_extract.hip and coeb_match.hip.  There is no CPU fallback: without a usable gfx950 device
// coeb_create fails.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "coeb_ctx.hpp"
#include "coeb_single_frame_host.hpp"
#include "coeb_rgbd_stream_host.hpp"

static const int8_t kPattern[1024] = {
#include "../../data/orb_bit_pattern_31.inc"
};

// per host thread: ranks of `bench.py --gpus N` (one thread per device) and threaded adapters call
// the library concurrently; coeb_last_error(NULL) returns the calling thread's last message
static thread_local std::string g_last_error;

constexpr int kFrameTmCap = 1024;     // T_M points per frame kept on the device (coeb_frame_batch_device)

void prof_begin(ProfileHook* p, const char* name, hipStream_t s)
{
    if (!p || !p->impl) return;
    ProfImpl* pi = static_cast<ProfImpl*>(p->impl);
    if (!pi->enabled) return;
    int id = -1;
    for (size_t i = 0; i < pi->names.size(); i++)
        if (pi->names[i] == name) id = (int)i;
    if (id < 0) {
        id = (int)pi->names.size();
        pi->names.push_back(name);
        pi->ms.push_back(0.0);
        pi->launches.push_back(0);
    }
    pi->cur_name = id;
    pi->cur_start = pi->get();
    (void)hipEventRecord(pi->cur_start, s);
}

void prof_end(ProfileHook* p, hipStream_t s)
{
    if (!p || !p->impl) return;
    ProfImpl* pi = static_cast<ProfImpl*>(p->impl);
    if (!pi->enabled || pi->cur_name < 0) return;
    hipEvent_t e = pi->get();
    (void)hipEventRecord(e, s);
    pi->pending.push_back({pi->cur_name, {pi->cur_start, e}});
    pi->cur_name = -1;
    if (pi->pending.size() > 4096) pi->drain();
}

int set_err(coeb_ctx* c, int code, const std::string& msg)
{
    if (c) c->err = msg;
    g_last_error = msg;
    return code;
}

int hip_err(coeb_ctx* c, hipError_t e, const char* where)
{
    return set_err(c, COEB_EDEVICE, std::string(where) + ": " + hipGetErrorString(e));
}

namespace {

// One frame's results written straight into the context's page-locked buffer (its device
// alias): the keypoint count and the first min(count, guess) records and descriptors, so the
// host reads them after one synchronisation with no copy operations in between (each D2H copy
// op of the single-frame path cost 5-25 us plus its launch gap, profiles/r06/sf).
// the delivered records and descriptors, common to k_out_pack and k_frame_tail
__device__ __forceinline__ void out_pack_copy(const uint32_t* kps, const uint4* desc, int n, int t, int T, uint32_t* out_k,
                                              uint4* out_d)
{
    for (int i = t; i < 7 * n; i += T) out_k[i] = kps[i];          // 28-byte records
    for (int i = t; i < 2 * n; i += T) out_d[i] = desc[i];         // 32-byte rows
}

__global__ __launch_bounds__(256) void k_out_pack(const int* counts, const uint32_t* kps, const uint4* desc, int guess,
                                                  int* out_n, uint32_t* out_k, uint4* out_d)
{
    const int n = min(*counts, guess);
    const int t = blockIdx.x * 256 + threadIdx.x, T = gridDim.x * 256;
    if (t == 0) *out_n = *counts;
    out_pack_copy(kps, desc, n, t, T, out_k, out_d);
}

// k_out_pack's place in coeb_frame_rgbd: the rest of the Frame RGB-D constructor
// (Frame.cc:216-223) on the records the extraction left on the device, written to the same
// page-locked buffer.  Per keypoint: mvKeysUn (UndistortKeyPoints, :579-609; a copy when
// mDistCoef[0] == 0), and ComputeStereoFromRGBD (:820-842) with the depth looked up at the RAW
// keypoint and uRight formed from the UNDISTORTED x.  The depth rows stay in host memory (the
// buffer's device alias): ~1000 of W*H values are read, each converted as
// Tracking::GrabImageRGBD's convertTo would have (Tracking.cc:227).  The gather is issued before
// the undistortion, whose ~200 double operations cover its PCIe round trip.
struct FrameTail {
    const int* counts; const uint32_t* kps; const uint4* desc; int guess;
    int* out_n; uint32_t* out_k; uint4* out_d;
    uint32_t* out_kun;          // null: kp_un_out not asked for
    float* out_ur; float* out_dep;
    const uint8_t* depth;       // W values per row, rows packed
    int W, H, depth_u16, depth_copy, undistort;
    float depth_scale, bf;
    DistK dist;
};

__global__ __launch_bounds__(256) void k_frame_tail(FrameTail a)
{
    const int n = min(*a.counts, a.guess);
    const int t = blockIdx.x * 256 + threadIdx.x, T = gridDim.x * 256;
    if (t == 0) *a.out_n = *a.counts;
    for (int i = t; i < n; i += T) {
        uint32_t r[7];
#pragma unroll
        for (int q = 0; q < 7; q++) r[q] = a.kps[7 * i + q];
        const float x = __uint_as_float(r[0]), y = __uint_as_float(r[1]);
        // imDepth.at<float>(v, u) with v = kp.pt.y, u = kp.pt.x (:829-832); keypoints lie inside
        // the image, the clamp only keeps a bad record from reading outside the staged rows
        const int px = min(max((int)x, 0), a.W - 1), py = min(max((int)y, 0), a.H - 1);
        const int64_t p = (int64_t)py * a.W + px;
        float d;
        if (a.depth_u16) {
            d = (float)reinterpret_cast<const uint16_t*>(a.depth)[p] * a.depth_scale;
        } else {
            d = reinterpret_cast<const float*>(a.depth)[p];
            if (!a.depth_copy) d = d * a.depth_scale;      // convertTo(CV_32F, scale): float product
        }
        float ux = x, uy = y;
        if (a.undistort) undistort_point(a.dist, ux, uy);
        if (a.out_kun) {
            a.out_kun[7 * i] = __float_as_uint(ux);
            a.out_kun[7 * i + 1] = __float_as_uint(uy);
#pragma unroll
            for (int q = 2; q < 7; q++) a.out_kun[7 * i + q] = r[q];
        }
        float ur = -1.f, dep = -1.f;
        if (d > 0) { dep = d; ur = ux - a.bf / d; }        // NaN and d <= 0 fail `d > 0` (:834)
        a.out_ur[i] = ur;
        a.out_dep[i] = dep;
    }
    out_pack_copy(a.kps, a.desc, n, t, T, a.out_k, a.out_d);
}

}  // namespace

int pinned(coeb_ctx* c, size_t bytes)
{
    if (c->pin_n >= bytes) return 0;
    if (c->pin) (void)hipHostFree(c->pin);
    c->pin = nullptr;
    c->pin_n = 0;
    const size_t n = std::max<size_t>(bytes, (size_t)1 << 20);
    hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&c->pin), n, hipHostMallocDefault);
    if (e != hipSuccess) return set_err(c, COEB_ENOMEM, std::string("hipHostMalloc: ") + hipGetErrorString(e));
    void* dv = nullptr;
    e = hipHostGetDevicePointer(&dv, c->pin, 0);
    if (e != hipSuccess) {
        (void)hipHostFree(c->pin);
        c->pin = nullptr;
        return set_err(c, COEB_ENOMEM, std::string("hipHostGetDevicePointer: ") + hipGetErrorString(e));
    }
    c->pin_dev = static_cast<uint8_t*>(dv);
    c->pin_n = n;
    return 0;
}

// pack -> pinned -> one H2D copy into the "stage" device buffer; *dbase = its device address.
// The previous call's copies have completed: every host-buffer entry point synchronises.
int stage_in(coeb_ctx* c, const Pack& pk, uint8_t** dbase, hipStream_t s)
{
    int rc;
    const size_t total = std::max<size_t>(pk.total, 16);
    if ((rc = pinned(c, total)) || (rc = ensure(c, c->ex.stage, total))) return rc;
    *dbase = c->ex.stage.p;
    size_t off = 0;
    for (const Pack::Part& q : pk.parts) {
        if (q.n) {
            if (q.p) memcpy(c->pin + off, q.p, q.n);
            else memset(c->pin + off, q.fill, q.n);
        }
        off = (off + q.n + 15) & ~(size_t)15;
    }
    HIP_TRY(c, hipMemcpyAsync(*dbase, c->pin, total, hipMemcpyHostToDevice, s));
    return 0;
}

namespace {
int err_word_async(coeb_ctx* c, uint8_t* dst);
int err_word_seen(coeb_ctx* c, const uint8_t* src);
}  // namespace

int Staged::stage(coeb_ctx* c, hipStream_t s, bool with_err)
{
    int rc;
    if ((rc = pinned(c, end() + (with_err ? 16 : 0))) || (rc = ensure(c, c->ex.stage, end())) || (rc = stage_in(c, pk, &dbase, s)))
        return rc;
    pin = c->pin;
    return 0;
}

int Staged::finish(coeb_ctx* c, hipStream_t s, size_t from, size_t to, bool with_err)
{
    int rc;
    HIP_TRY(c, hipMemcpyAsync(pin + from, dbase + from, to - from, hipMemcpyDeviceToHost, s));
    if (with_err && (rc = err_word_async(c, pin + end()))) return rc;
    HIP_TRY(c, hipStreamSynchronize(s));
    if (with_err && (rc = err_word_seen(c, pin + end()))) return rc;
    return 0;
}

namespace {

int ensure_plan(coeb_ctx* c, int W, int H)
{
    if (c->has_plan && c->plan.W == W && c->plan.H == H) return 0;
    if (W <= 0 || H <= 0 || W > c->max_w || H > c->max_h)
        return set_err(c, COEB_EINVAL, "image size outside the context limits");
    std::string err;
    Plan P;
    if (!make_plan(c->tab, W, H, 0, P, c->rtab, c->cells, err)) return set_err(c, COEB_EINVAL, err);
    // the plan, rtab and cells are rewritten in place below: batches still in flight on the
    // context's streams (pyramid / FAST / octree / describe read them) must finish first
    int rc;
    if ((rc = quiesce(c))) return rc;
    c->plan = P;
    PlanBufs& d = c->pl;
    if ((rc = ensure(c, d.plan, 1)) || (rc = ensure(c, d.rtab, std::max<size_t>(c->rtab.size(), 1))) ||
        (rc = ensure(c, d.cells, c->cells.size())) || (rc = ensure(c, d.pattern, 1024)))
        return rc;
    HIP_TRY(c, hipMemcpy(d.plan.p, &c->plan, sizeof(Plan), hipMemcpyHostToDevice));
    if (!c->rtab.empty()) HIP_TRY(c, hipMemcpy(d.rtab.p, c->rtab.data(), c->rtab.size() * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(d.cells.p, c->cells.data(), c->cells.size() * sizeof(CellDesc), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(d.pattern.p, kPattern, 1024, hipMemcpyHostToDevice));
    c->has_plan = true;
    return 0;
}

// Allocate per-frame buffers for F frames and fill ExtractBufs.
int extract_bufs(coeb_ctx* c, int F, ExtractBufs& b)
{
    const Plan& P = c->plan;
    memset(&b, 0, sizeof(b));
    int rc;
    ExtractDev& d = c->ex;
    if ((rc = ensure(c, d.pyr, (size_t)F * P.pyr_stride + 4096)) || (rc = ensure(c, d.blur, (size_t)F * P.blur_stride + 4096)) ||
        (rc = ensure(c, d.cand_n, (size_t)F * P.ncells)) || (rc = ensure(c, d.cand, (size_t)F * P.ncells * P.cell_cap)) ||
        (rc = ensure(c, d.keys, (size_t)F * 2 * P.kbuf_stride)) || (rc = ensure(c, d.nodes, (size_t)F * P.node_stride * 4)) ||
        (rc = ensure(c, d.lvl_n, (size_t)F * P.L)) || (rc = ensure(c, d.lvl_kp, (size_t)F * P.lvl_stride)) ||
        (rc = ensure(c, d.kps, (size_t)F * P.kcap)) || (rc = ensure(c, d.desc, (size_t)F * P.kcap * 32)) ||
        (rc = ensure(c, d.counts, (size_t)F)) || (rc = ensure(c, d.dyn, (size_t)F)) || (rc = ensure(c, d.err, 4)))
        return rc;
    b.pyr = d.pyr.p; b.blur = d.blur.p; b.cand_n = d.cand_n.p; b.cand = d.cand.p; b.keys = d.keys.p; b.nodes = d.nodes.p;
    b.lvl_n = d.lvl_n.p; b.lvl_kp = d.lvl_kp.p; b.kps = d.kps.p; b.desc = d.desc.p; b.counts = d.counts.p; b.dyn = d.dyn.p;
    b.err = d.err.p; b.rtab = c->pl.rtab.p; b.cells = c->pl.cells.p; b.pattern = c->pl.pattern.p;
    return 0;
}

// Upload per-frame boxes / T_M / blur flags (host arrays, offset layout) for F frames.
int upload_dyn(coeb_ctx* c, int F, const coeb_box* boxes, const int32_t* box_off, const float* tm_xy,
               const int32_t* tm_off, const int32_t* blur_flag, ExtractBufs& b)
{
    const int nbox = (box_off && boxes) ? box_off[F] : 0;
    const int ntm = (tm_off && tm_xy) ? tm_off[F] : 0;
    int rc;
    ExtractDev& d = c->ex;
    // offsets must start at 0 and never decrease: every box then gets its frame from
    // k_box_frame, and every T_M range lies inside the uploaded array
    if (box_off && boxes && box_off[0] != 0) return set_err(c, COEB_EINVAL, "box_off[0] != 0");
    if (tm_off && tm_xy && tm_off[0] != 0) return set_err(c, COEB_EINVAL, "tm_off[0] != 0");
    for (int f = 0; f < F; f++) {
        if (box_off && boxes && box_off[f + 1] < box_off[f]) return set_err(c, COEB_EINVAL, "box_off decreases");
        if (tm_off && tm_xy && tm_off[f + 1] < tm_off[f]) return set_err(c, COEB_EINVAL, "tm_off decreases");
    }
    if (nbox > 0) {
        for (int f = 0; f < F; f++)
            if (box_off[f + 1] - box_off[f] > COEB_MAXBOX) return set_err(c, COEB_EINVAL, "more than 16 boxes in a frame");
        if ((rc = ensure(c, d.boxes, (size_t)nbox * 4)) || (rc = ensure(c, d.box_off, (size_t)F + 1)) ||
            (rc = ensure(c, d.blurf, (size_t)nbox)))
            return rc;
        HIP_TRY(c, hipMemcpyAsync(d.boxes.p, boxes, (size_t)nbox * 16, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(d.box_off.p, box_off, (size_t)(F + 1) * 4, hipMemcpyHostToDevice, c->stream));
        if (blur_flag) {
            HIP_TRY(c, hipMemcpyAsync(d.blurf.p, blur_flag, (size_t)nbox * 4, hipMemcpyHostToDevice, c->stream));
        } else {
            HIP_TRY(c, hipMemsetAsync(d.blurf.p, 0, (size_t)nbox * 4, c->stream));
        }
        b.boxes = d.boxes.p; b.box_off = d.box_off.p; b.blurf = d.blurf.p;
    }
    if (ntm > 0) {
        if ((rc = ensure(c, d.tm, (size_t)ntm * 2)) || (rc = ensure(c, d.tm_off, (size_t)F + 1))) return rc;
        HIP_TRY(c, hipMemcpyAsync(d.tm.p, tm_xy, (size_t)ntm * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(d.tm_off.p, tm_off, (size_t)(F + 1) * 4, hipMemcpyHostToDevice, c->stream));
        b.tm = d.tm.p; b.tm_off = d.tm_off.p;
    }
    return 0;
}

}  // namespace

// The product switches (coeb_internal.hpp); every one of them is set by a GPU test.
static const char* const kSwitches[] = {
    "COEB_SIDE_STREAM",        // 0: no extraction side stream     (test_sharded_batch_equals_unsharded[off])
    "COEB_SIDE_SHARED",        // 1: one side stream per device     ([shared], bench config C)
    "COEB_SIDE_EAGER",         // 1: side stream made with the ctx  ([eager], bench config A)
    "COEB_MATCH_SEQUENTIAL",   // 1: the literal sequential claims  (test_match_paths_agree, ...)
    "COEB_MATCH_SPLIT",        // N: split-list workgroups per pair (test_batch_small_split_lists...)
    "COEB_PYR_BYTES",          // 1: k_pyr_level byte form          (test_blur_pyramid_matches_oracle)
    "COEB_FAST_RB",            // 72: the general FAST slab layout  (test_fast_general_slab_layout...)
    "COEB_FM_THREADS",         // k_fm threads per pair             (tests/test_gpu_flow.py)
};

const char* coeb_switch(const char* name)
{
    for (const char* k : kSwitches)
        if (strcmp(k, name) == 0) return getenv(name);
    return nullptr;            // not a product switch: never read
}

namespace {

// The device's shared side stream (COEB_SIDE_SHARED=1): with P pipelines the P context streams
// plus one side stream fill the 4 hardware queues exactly, instead of 2P streams sharing them.
// Reference-counted over the contexts that use it.
static std::mutex g_shared_side_mu;
static std::map<int, std::pair<hipStream_t, int>> g_shared_side;

static hipError_t shared_side_acquire(int device, hipStream_t* out)
{
    std::lock_guard<std::mutex> lk(g_shared_side_mu);
    auto& e = g_shared_side[device];
    if (!e.first) {
        hipError_t r = hipStreamCreateWithFlags(&e.first, hipStreamNonBlocking);
        if (r != hipSuccess) { e.first = nullptr; return r; }
    }
    ++e.second;
    *out = e.first;
    return hipSuccess;
}

static void shared_side_release(int device)
{
    std::lock_guard<std::mutex> lk(g_shared_side_mu);
    auto it = g_shared_side.find(device);
    if (it == g_shared_side.end() || --it->second.second > 0) return;
    (void)hipStreamSynchronize(it->second.first);
    (void)hipStreamDestroy(it->second.first);
    g_shared_side.erase(it);
}

}  // namespace

// The side stream of launch_extract (created on first use), or null when disabled.  Per-kernel
// profiling (coeb_profile_enable) serialises everything on the context stream, so each event
// pair brackets one whole-batch launch.
const SideStream* side_stream(coeb_ctx* c)
{
    if (c->prof.enabled) return nullptr;
    if (!c->side_init) {
        c->side_init = true;
        const char* e = coeb_switch("COEB_SIDE_STREAM");
        if (e && e[0] == '0') return nullptr;
        const char* sh = coeb_switch("COEB_SIDE_SHARED");         // 1: one side stream per device
        c->side_shared = sh && sh[0] == '1';
        hipError_t se = c->side_shared ? shared_side_acquire(c->device, &c->side.s)
                                       : hipStreamCreateWithFlags(&c->side.s, hipStreamNonBlocking);
        hipEvent_t* evs[] = {&c->side.fork, &c->side.mid, &c->side.pyr_done, &c->side.join};
        bool ok = se == hipSuccess;
        for (hipEvent_t* e : evs) {
            *e = nullptr;
            if (ok && hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess) {
                *e = nullptr;
                ok = false;
            }
        }
        if (!ok) {
            // run without a side stream: release what was made
            for (hipEvent_t* e : evs)
                if (*e) (void)hipEventDestroy(*e), *e = nullptr;
            if (se == hipSuccess) {
                if (c->side_shared) shared_side_release(c->device);
                else (void)hipStreamDestroy(c->side.s);
            }
            c->side.s = nullptr;
            c->side_shared = false;
        }
    }
    return c->side.s ? &c->side : nullptr;
}

// The context stream waits for the last batch pose (k_pose on pose_stream).
void join_pose(coeb_ctx* c)
{
    if (c->pose_pending) {
        (void)hipStreamWaitEvent(c->stream, c->ev_pose, 0);
        c->pose_pending = false;
    }
}

hipStream_t main_stream(coeb_ctx* c)
{
    if (c->pending_join) {
        for (hipStream_t s : c->subs) {
            (void)hipEventRecord(c->ev_join, s);
            (void)hipStreamWaitEvent(c->stream, c->ev_join, 0);
        }
        c->pending_join = false;
    }
    return c->stream;
}

// Wait until nothing enqueued by this context is still running: the chunk streams and the pose
// stream are joined into the context stream (the side stream is joined there by every
// extraction), then the context stream is drained.
int quiesce(coeb_ctx* c)
{
    if (!c->stream) return 0;
    main_stream(c);
    join_pose(c);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return 0;
}

namespace {

// Chunk boundaries for F frames over the context's batch streams (>= 16 frames per chunk).
int make_chunks(coeb_ctx* c, int F)
{
    int n = std::max(1, std::min(c->nstreams, F / 16));
    if (n > 1 && (int)c->subs.size() < n) {
        while ((int)c->subs.size() < n) {
            hipStream_t s;
            hipEvent_t a, b;
            if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) break;
            (void)hipEventCreateWithFlags(&a, hipEventDisableTiming);
            (void)hipEventCreateWithFlags(&b, hipEventDisableTiming);
            c->subs.push_back(s);
            c->ev_prep.push_back(a);
            c->ev_mdone.push_back(b);
        }
        n = std::min<int>(n, (int)c->subs.size());
    }
    c->chunk.assign(n + 1, 0);
    for (int k = 0; k <= n; k++) c->chunk[k] = (int)((int64_t)F * k / n);
    return n;
}

// Per-frame buffers of frames [f0, ...): every per-frame array advanced by f0 frames.
ExtractBufs offset_bufs(const Plan& P, const ExtractBufs& b, int f0)
{
    ExtractBufs o = b;
    o.gray = b.gray + (int64_t)f0 * P.W * P.H;
    o.pyr = b.pyr + (int64_t)f0 * P.pyr_stride;
    o.blur = b.blur + (int64_t)f0 * P.blur_stride;
    o.cand_n = b.cand_n + (int64_t)f0 * P.ncells;
    o.cand = b.cand + (int64_t)f0 * P.ncells * P.cell_cap;
    o.keys = b.keys + (int64_t)f0 * 2 * P.kbuf_stride;
    o.nodes = b.nodes + (int64_t)f0 * P.node_stride * 4;
    o.lvl_n = b.lvl_n + (int64_t)f0 * P.L;
    o.lvl_kp = b.lvl_kp + (int64_t)f0 * P.lvl_stride;
    o.kps = static_cast<coeb_keypoint*>(b.kps) + (int64_t)f0 * P.kcap;
    o.desc = b.desc + (int64_t)f0 * P.kcap * 32;
    o.counts = b.counts + f0;
    o.dyn = b.dyn + f0;
    if (b.box_off) o.box_off = b.box_off + f0;   // offsets index the shared box / T_M arrays
    if (b.tm_off) o.tm_off = b.tm_off + f0;
    return o;
}

// The device error word copied behind the work of a host-buffer call into `dst` (page-locked),
// so the call's one synchronisation also brings the word back; err_word_seen checks the copy.
int err_word_async(coeb_ctx* c, uint8_t* dst)
{
    if (!c->ex.err.p) {
        memset(dst, 0, 4);
        return 0;
    }
    HIP_TRY(c, hipMemcpyAsync(dst, c->ex.err.p, 4, hipMemcpyDeviceToHost, main_stream(c)));
    return 0;
}

// h: the error word as read back.  Non-zero: the device word is reset and the call fails.
int err_word_report(coeb_ctx* c, int h)
{
    if (!h) return 0;
    char msg[160];
    snprintf(msg, sizeof msg, "internal capacity exceeded (device error bits 0x%x)", h);
    HIP_TRY(c, hipMemsetAsync(c->ex.err.p, 0, 4, main_stream(c)));
    return set_err(c, COEB_ERANGE, msg);
}

int err_word_seen(coeb_ctx* c, const uint8_t* src)
{
    int h = 0;
    memcpy(&h, src, 4);
    return err_word_report(c, h);
}

// coeb_synchronize: the word fetched by a copy and a synchronisation of its own
int check_err_word(coeb_ctx* c)
{
    main_stream(c);
    if (!c->ex.err.p) return 0;
    int h = 0;
    HIP_TRY(c, hipMemcpyAsync(&h, c->ex.err.p, 4, hipMemcpyDeviceToHost, main_stream(c)));
    HIP_TRY(c, hipStreamSynchronize(main_stream(c)));
    return err_word_report(c, h);
}

// What coeb_extract and coeb_frame_rgbd enqueue on the context stream between pinned() and their
// output kernel: the gray rows through the page-locked buffer into gray_stage, the dynamic-mask
// inputs staged at L's offsets, and the extraction of the one frame; b holds its buffers.
// Pinned staging at both ends: the image rows go through the page-locked buffer (one DMA, no
// runtime pinning of the caller's pages), and the results come back into it behind the kernels
// (a pageable round trip each cost 120-170 us on the box, profiles/r06/sf).
int enqueue_single_frame(coeb_ctx* c, const SingleFrameLayout& L, const uint8_t* gray, int W, int H, size_t stride,
                         const coeb_box* boxes, int nbox, const float* tm_xy, int ntm, const int32_t* blur_flag, int nblur,
                         ExtractBufs& b)
{
    uint8_t* dgray = c->ex.gray_stage.p;
    hipStream_t s = main_stream(c);
    single_frame_stage_rows(c->pin, gray, H, (size_t)W, stride);
    HIP_TRY(c, hipMemcpyAsync(dgray, c->pin, (size_t)W * H, hipMemcpyHostToDevice, s));
    int32_t* box_off = reinterpret_cast<int32_t*>(c->pin + L.o_bo);
    int32_t* tm_off = reinterpret_cast<int32_t*>(c->pin + L.o_to);
    int32_t* blur = reinterpret_cast<int32_t*>(c->pin + L.o_bl);
    box_off[0] = 0; box_off[1] = nbox; tm_off[0] = 0; tm_off[1] = ntm;
    for (int i = 0; i < nbox; i++)                      // missing flags (or a null array) read as 0
        blur[i] = (blur_flag && i < nblur) ? blur_flag[i] : 0;
    if (nbox) memcpy(c->pin + L.o_dyn, boxes, (size_t)nbox * sizeof(coeb_box));
    if (ntm) memcpy(c->pin + L.o_tm, tm_xy, (size_t)ntm * 8);
    int rc;
    if ((rc = extract_bufs(c, 1, b))) return rc;
    if ((rc = upload_dyn(c, 1, nbox ? reinterpret_cast<const coeb_box*>(c->pin + L.o_dyn) : nullptr, box_off,
                         ntm ? reinterpret_cast<const float*>(c->pin + L.o_tm) : nullptr, tm_off, nbox ? blur : nullptr, b)))
        return rc;
    b.gray = dgray;
    // one frame on one stream: the side stream's fork / join cost more than the overlap it buys
    // at F = 1 (0.389 vs 0.350 ms per single-frame step, profiles/r06/sf)
    if (launch_extract(c->plan, c->pl.plan.p, b, 1, s, &c->hook, nullptr))
        return hip_err(c, hipGetLastError(), "launch_extract");
    c->batch_frames = 1;
    c->batch_gray = dgray;
    return 0;
}

// Behind the output kernel: the error word, the call's one synchronisation, and the keypoint
// count the kernel left at L.o_n.
int finish_single_frame(coeb_ctx* c, const SingleFrameLayout& L, hipStream_t s, int* n)
{
    int rc;
    if ((rc = err_word_async(c, c->pin + L.o_n + 16))) return rc;
    HIP_TRY(c, hipStreamSynchronize(s));
    if ((rc = err_word_seen(c, c->pin + L.o_n + 16))) return rc;
    memcpy(n, c->pin + L.o_n, 4);
    return 0;
}

// the projection searches' result as the caller takes it: hout = match[cs], nmatch
void match_copy_out(const int32_t* hout, int n, int cs, int32_t* match_out, int* nmatches)
{
    if (n && match_out) memcpy(match_out, hout, (size_t)n * 4);
    *nmatches = hout[cs];
}

// scratch of coeb_match_localmap / coeb_match_keyframe (qs points) and the error word they read
int projection_bufs(coeb_ctx* c, int qs)
{
    SingleFrameBufs& sf = c->sf;
    int rc;
    if ((rc = ensure(c, sf.l_list, (size_t)qs * kCQ)) || (rc = ensure(c, c->ex.err, 4)) || (rc = ensure(c, sf.l_path, 2)))
        return rc;
    return 0;
}

// ---- shared by the single-frame tracking calls ----
// Each of them works in one staged region (Staged, coeb_ctx.hpp): the inputs are packed and uploaded
// in one copy, the results that have an initial value (counts, the pose) last among them; the results
// the kernels write follow, so that one copy brings every result back; scratch comes last.  A call
// reads as what differs: which arrays go in, which kernels run, which results come back.

// the current frame's mvKeysUn, mDescriptors and mvuRight, consecutive in the staged inputs
struct CurOff { size_t k, d, ur; };
CurOff pack_cur(Staged& st, const coeb_curframe* cur)
{
    const size_t n = (size_t)cur->n;
    CurOff o;
    o.k = st.add(cur->keys_un, n * sizeof(coeb_keypoint));
    o.d = st.add(cur->descriptors, n * 32);
    o.ur = st.add(cur->u_right, n * 4);
    return o;
}

// every one of the n keypoints lies on a pyramid level (the kernels index the per-level tables with it)
bool octaves_in_pyramid(const coeb_ctx* c, const coeb_keypoint* kps, int n)
{
    for (int i = 0; i < n; i++)
        if (kps[i].octave < 0 || kps[i].octave >= c->tab.nlevels) return false;
    return true;
}

// k_pose's scratch for `count` keypoints in all
int pose_scratch(coeb_ctx* c, size_t count)
{
    SingleFrameBufs& sf = c->sf;
    int rc;
    if ((rc = ensure(c, sf.p_act, count)) || (rc = ensure(c, sf.p_edge, count)) || (rc = ensure(c, sf.p_chi, count))) return rc;
    return 0;
}

// k_pose's arguments over device arrays, on pose_scratch()'s buffers
PoseBufs pose_bufs(coeb_ctx* c, const int* n, const uint8_t* has, const float* xw, const void* kps, const float* ur,
                   const float* inv_sigma2, float* Tcw, uint8_t* outlier, int* result, int stride)
{
    PoseBufs b;
    b.n = n; b.has_mp = has; b.xw = xw; b.kps = kps; b.ur = ur; b.inv_sigma2 = inv_sigma2; b.Tcw = Tcw;
    b.outlier = outlier; b.result = result; b.edges = c->sf.p_edge.p; b.active = c->sf.p_act.p; b.chi2 = c->sf.p_chi.p;
    b.stride = stride; b.timing = nullptr;
    return b;
}

// The current / last frame pair of SearchByProjection(CurrentFrame, LastFrame), as coeb_match_lastframe
// and coeb_track_motion_model stage it: {n, nl}, the two poses, the current frame, the last frame's
// six arrays.
bool last_arrays_missing(const coeb_lastframe* last)
{
    return last->n && (!last->has_mappoint || !last->outlier || !last->world_pos || !last->mp_descriptor ||
                       !last->mp_observations || !last->keys_un);
}

struct LastPair {
    int32_t cnts[2];            // uploaded from here: lives as long as the Pack
    size_t cn, T, Tl, lk, ld, h, o, xw, nb;
    CurOff cur;
};
void pack_last_pair(Staged& st, const coeb_curframe* cur, const coeb_lastframe* last, const float* Tcw_cur,
                    const float* Tcw_last, LastPair& p)
{
    const size_t nl = (size_t)last->n;
    p.cnts[0] = cur->n; p.cnts[1] = last->n;
    p.cn = st.add(p.cnts, 8); p.T = st.add(Tcw_cur, 64); p.Tl = st.add(Tcw_last, 64);
    p.cur = pack_cur(st, cur);
    p.lk = st.add(last->keys_un, nl * sizeof(coeb_keypoint));
    p.ld = st.add(last->mp_descriptor, nl * 32); p.h = st.add(last->has_mappoint, nl);
    p.o = st.add(last->outlier, nl); p.xw = st.add(last->world_pos, nl * 12);
    p.nb = st.add(last->mp_observations, nl * 4);
}

// k_match's arguments for that pair, all but where match / nmatch live; m_scr, m_qn and the error
// word have been ensured for ls LastFrame slots.  One pair: its candidate lists are built by 8
// workgroups (k_match_lists), as for a small batch, instead of by the pair's one workgroup.
MatchBufs last_pair_bufs(coeb_ctx* c, const Staged& st, const LastPair& p, int cs, int ls)
{
    MatchBufs mb;
    memset(&mb, 0, sizeof(mb));
    mb.cur_kps = st.dev<void>(p.cur.k); mb.cur_desc = st.dev<uint8_t>(p.cur.d); mb.cur_n = st.dev<int32_t>(p.cn);
    mb.cur_ur = st.dev<float>(p.cur.ur); mb.cur_stride = cs;
    mb.last_kps = st.dev<void>(p.lk); mb.last_desc = st.dev<uint8_t>(p.ld); mb.last_n = st.dev<int32_t>(p.cn) + 1;
    mb.last_has = st.dev<uint8_t>(p.h); mb.last_out = st.dev<uint8_t>(p.o); mb.last_xw = st.dev<float>(p.xw);
    mb.last_nobs = st.dev<int32_t>(p.nb); mb.last_stride = ls;
    mb.Tcw_cur = st.dev<float>(p.T); mb.Tcw_last = st.dev<float>(p.Tl);
    mb.scratch = c->sf.m_scr.p; mb.scratch_stride = ls * kCQ; mb.err = c->ex.err.p;
    mb.qn = c->sf.m_qn.p; mb.qn_stride = ls + kMaxSplit;
    return mb;
}

}  // namespace

// declared in coeb_ctx.hpp: coeb_kfdb.hip calls it too
MatchCam make_cam(const coeb_ctx* c, const coeb_camera* cam)
{
    MatchCam m;
    memset(&m, 0, sizeof(m));
    m.fx = cam->fx; m.fy = cam->fy; m.cx = cam->cx; m.cy = cam->cy; m.bf = cam->bf;
    m.mb = cam->bf / cam->fx;                                       // Frame.cc:246
    m.min_x = cam->min_x; m.max_x = cam->max_x; m.min_y = cam->min_y; m.max_y = cam->max_y;
    m.grid_inv_w = (float)COEB_GRID_COLS / (cam->max_x - cam->min_x);   // Frame.cc:233-234
    m.grid_inv_h = (float)COEB_GRID_ROWS / (cam->max_y - cam->min_y);
    for (int l = 0; l < c->tab.nlevels; l++) m.scale[l] = c->tab.scale[l];
    m.nlevels = c->tab.nlevels;
    // mfLogScaleFactor = log(mfScaleFactor): std::log(float), canonical correctly rounded
    m.log_sf = (float)std::log((double)(float)c->tab.scale_factor);
    return m;
}

extern "C" {

int coeb_abi_version(void) { return COEB_ABI_VERSION; }

int coeb_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

coeb_ctx* coeb_create(const coeb_orb_params* params, int device, int max_width, int max_height, int max_batch)
{
    if (!params || max_width <= 0 || max_height <= 0 || max_batch <= 0) {
        g_last_error = "coeb_create: invalid arguments";
        return nullptr;
    }
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) {
        g_last_error = "coeb_create: no usable HIP device (the HIP path has no CPU fallback)";
        return nullptr;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        g_last_error = std::string("coeb_create: device is not gfx950 (") + prop.gcnArchName + ")";
        return nullptr;
    }
    coeb_ctx* c = new coeb_ctx();
    c->device = device;
    c->params = *params;
    if (!make_tables(*params, c->tab)) {
        g_last_error = "coeb_create: invalid ORB parameters";
        delete c;
        return nullptr;
    }
    c->max_w = max_width;
    c->max_h = max_height;
    c->max_batch = max_batch;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        g_last_error = "coeb_create: stream creation failed";
        delete c;
        return nullptr;
    }
    c->hook.impl = &c->prof;
    // COEB_SIDE_EAGER=1: create the side stream now, right after the context stream, so the
    // contexts' streams take the hardware queues in (context, side) pairs (experiment knob; by
    // default it is created at the first extraction, after every context stream of the process)
    if (const char* e = coeb_switch("COEB_SIDE_EAGER"))
        if (e[0] == '1') (void)side_stream(c);
    if (hipEventCreateWithFlags(&c->ev_main, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess) {
        g_last_error = "coeb_create: event creation failed";
        coeb_destroy(c);
        return nullptr;
    }
    if (ensure(c, c->ex.err, 4) || hipMemset(c->ex.err.p, 0, 16) != hipSuccess) {
        g_last_error = "coeb_create: device allocation failed";
        coeb_destroy(c);
        return nullptr;
    }
    return c;
}

void coeb_destroy(coeb_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(main_stream(c));
    if (c->side.s) {
        if (c->side_shared) {
            // this context's side work ends at its join event; the other contexts' work queued on
            // the shared stream is theirs to wait for (the last release synchronises the stream)
            (void)hipEventSynchronize(c->side.join);
            shared_side_release(c->device);
        } else {
            (void)hipStreamSynchronize(c->side.s);
            (void)hipStreamDestroy(c->side.s);
        }
        (void)hipEventDestroy(c->side.fork);
        (void)hipEventDestroy(c->side.mid);
        (void)hipEventDestroy(c->side.pyr_done);
        (void)hipEventDestroy(c->side.join);
    }
    if (c->pose_stream) {
        (void)hipStreamSynchronize(c->pose_stream);
        (void)hipStreamDestroy(c->pose_stream);
        (void)hipEventDestroy(c->ev_tprep);
        (void)hipEventDestroy(c->ev_pose);
        if (c->ev_tlm) (void)hipEventDestroy(c->ev_tlm);
    }
    kfdb_release_all(c);
    auto free_buf = [](auto& a) { if (a.p) (void)hipFree(a.p); };
    each_buf(c->pl, free_buf); each_buf(c->ex, free_buf); each_buf(c->fb, free_buf);
    each_buf(c->bm, free_buf); each_buf(c->bp, free_buf); each_buf(c->tl, free_buf);
    each_buf(c->sf, free_buf); each_buf(c->tim, free_buf); each_buf(c->hl, free_buf);
    each_buf(c->bow, free_buf);
    c->prof.drain();
    for (auto e : c->prof.pool) (void)hipEventDestroy(e);
    for (size_t k = 0; k < c->subs.size(); k++) {
        (void)hipStreamDestroy(c->subs[k]);
        (void)hipEventDestroy(c->ev_prep[k]);
        (void)hipEventDestroy(c->ev_mdone[k]);
    }
    if (c->ev_main) (void)hipEventDestroy(c->ev_main);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    if (c->pin) (void)hipHostFree(c->pin);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

const char* coeb_last_error(const coeb_ctx* c)
{
    if (c && !c->err.empty()) return c->err.c_str();
    return g_last_error.c_str();
}

int coeb_orb_tables_get(const coeb_ctx* c, coeb_orb_tables* out)
{
    if (!c || !out) return COEB_EINVAL;
    memset(out, 0, sizeof(*out));
    out->nlevels = c->tab.nlevels;
    out->scale_factor = (float)c->tab.scale_factor;
    for (int l = 0; l < c->tab.nlevels; l++) {
        out->scale[l] = c->tab.scale[l];
        out->inv_scale[l] = c->tab.inv_scale[l];
        out->sigma2[l] = c->tab.sigma2[l];
        out->inv_sigma2[l] = c->tab.inv_sigma2[l];
        out->features_per_level[l] = c->tab.nfeat[l];
    }
    memcpy(out->umax, c->tab.umax, sizeof(out->umax));
    return COEB_OK;
}

int coeb_max_keypoints(const coeb_ctx* cc, int width, int height)
{
    coeb_ctx* c = const_cast<coeb_ctx*>(cc);
    if (!c) return COEB_EINVAL;
    (void)hipSetDevice(c->device);
    int rc = ensure_plan(c, width, height);
    if (rc) return rc;
    return c->plan.kcap;
}

int coeb_extract_batch_device(coeb_ctx* c, const uint8_t* d_gray, int F, int W, int H, const coeb_box* boxes,
                              const int32_t* box_off, const float* tm_xy, const int32_t* tm_off,
                              const int32_t* blur_flag)
{
    if (!c || !d_gray || F <= 0) return set_err(c, COEB_EINVAL, "coeb_extract_batch_device: invalid arguments");
    if (F > c->max_batch) return set_err(c, COEB_EINVAL, "batch larger than max_batch");
    (void)hipSetDevice(c->device);
    int rc;
    if ((rc = ensure_plan(c, W, H))) return rc;
    ExtractBufs b;
    const std::vector<int> prev_chunk = c->chunk;
    const bool prev_mdone = c->mdone_valid;
    const int n = make_chunks(c, F);
    const bool has_dyn = (boxes && box_off) || (tm_xy && tm_off);
    // per-frame buffers may be reallocated and the box / T_M staging rewritten: let every
    // outstanding batch finish first in those cases
    const bool serial = n == 1 || has_dyn || (c->batch_frames != F);
    if (serial) main_stream(c);
    if ((rc = extract_bufs(c, F, b))) return rc;
    if ((rc = upload_dyn(c, F, boxes, box_off, tm_xy, tm_off, blur_flag, b))) return rc;
    b.gray = d_gray;
    const Plan* dplan = c->pl.plan.p;
    c->mdone_valid = false;
    c->extract_chunked = n > 1;
    if (n == 1) {
        if (launch_extract(c->plan, dplan, b, F, main_stream(c), &c->hook, side_stream(c)))
            return hip_err(c, hipGetLastError(), "launch_extract");
    } else {
        HIP_TRY(c, hipEventRecord(c->ev_main, c->stream));   // no join: steps overlap
        const bool cross = !serial && prev_mdone && prev_chunk == c->chunk;
        for (int k = 0; k < n; k++) {
            hipStream_t s = c->subs[k];
            HIP_TRY(c, hipStreamWaitEvent(s, c->ev_main, 0));
            // the previous batch's matcher of chunk k+1 reads chunk k's last frame
            if (cross && k + 1 < n) HIP_TRY(c, hipStreamWaitEvent(s, c->ev_mdone[k + 1], 0));
            const int f0 = c->chunk[k], f1 = c->chunk[k + 1];
            if (launch_extract(c->plan, dplan, offset_bufs(c->plan, b, f0), f1 - f0, s, &c->hook))
                return hip_err(c, hipGetLastError(), "launch_extract");
        }
        c->pending_join = true;
    }
    c->batch_frames = F;
    c->batch_gray = d_gray;
    return COEB_OK;
}

int coeb_frame_batch_device(coeb_ctx* c, const uint8_t* d_gray, int F, int W, int H, const coeb_box* boxes,
                            const int32_t* box_off)
{
    if (!c || !d_gray || F <= 0 || (boxes && !box_off))
        return set_err(c, COEB_EINVAL, "coeb_frame_batch_device: invalid arguments");
    if (F > c->max_batch) return set_err(c, COEB_EINVAL, "batch larger than max_batch");
    (void)hipSetDevice(c->device);
    int rc;
    if ((rc = ensure_plan(c, W, H))) return rc;
    // Everything below runs on the context stream, so stream order protects the flow scratch,
    // T_M and the box staging of the previous batch (ensure() quiesces before it reallocates);
    // the pose stream reads only its own snapshots (k_track_prep / k_tlm_snapshot).
    hipStream_t s = main_stream(c);
    const int nbox = boxes ? box_off[F] : 0;
    FrameBatchBufs& fb = c->fb;
    if ((rc = ensure(c, fb.f_tm, (size_t)F * kFrameTmCap * 2)) || (rc = ensure(c, fb.f_ntm, (size_t)F))) return rc;
    // ProcessMovingObject(frame f-1, frame f) -> T_M of frame f (Frame.cc:164-166)
    if ((rc = pmo_batch(c, d_gray, F, W, H, fb.f_tm.p, fb.f_ntm.p, kFrameTmCap))) return rc;
    ExtractBufs b;
    if ((rc = extract_bufs(c, F, b))) return rc;
    if ((rc = upload_dyn(c, F, boxes, box_off, nullptr, nullptr, nullptr, b))) return rc;
    if (nbox > 0) {
        // detect_laplacian blur flag of every box (Frame.cc:171-202); frame 0 = the first frame.
        // The box -> frame map is built on the device from the box offsets upload_dyn staged.
        if ((rc = ensure(c, fb.f_bframe, (size_t)nbox)) || (rc = ensure(c, fb.f_blur, (size_t)nbox))) return rc;
        if (blur_flags_batch(c, d_gray, W, H, b.boxes, b.box_off, F, fb.f_bframe.p, nbox, fb.f_blur.p, s))
            return hip_err(c, hipGetLastError(), "blur flags");
        b.blurf = fb.f_blur.p;
    }
    b.tmd = fb.f_tm.p;
    b.ntmd = fb.f_ntm.p;
    b.tmd_cap = kFrameTmCap;
    b.gray = d_gray;
    c->mdone_valid = false;
    c->extract_chunked = false;
    c->chunk.assign(2, 0);
    c->chunk[1] = F;
    if (launch_extract(c->plan, c->pl.plan.p, b, F, s, &c->hook, side_stream(c)))
        return hip_err(c, hipGetLastError(), "launch_extract");
    c->batch_frames = F;
    c->batch_gray = d_gray;
    return COEB_OK;
}

int coeb_batch_frame_results(coeb_ctx* c, const float** d_tm, const int32_t** d_ntm, int* tm_cap,
                             const int32_t** d_blur)
{
    if (!c || !c->fb.f_ntm.p) return set_err(c, COEB_EINVAL, "no frame batch yet");
    if (d_tm) *d_tm = c->fb.f_tm.p;
    if (d_ntm) *d_ntm = c->fb.f_ntm.p;
    if (tm_cap) *tm_cap = kFrameTmCap;
    if (d_blur) *d_blur = c->fb.f_blur.p;
    return COEB_OK;
}

int coeb_set_batch_streams(coeb_ctx* c, int nstreams)
{
    if (!c || nstreams < 1 || nstreams > 16) return set_err(c, COEB_EINVAL, "coeb_set_batch_streams: 1..16 streams");
    (void)hipSetDevice(c->device);
    main_stream(c);
    c->nstreams = nstreams;
    c->mdone_valid = false;
    return COEB_OK;
}

int coeb_batch_results(coeb_ctx* c, const coeb_keypoint** d_kps, const uint8_t** d_desc, const int32_t** d_counts,
                       int* kcap)
{
    if (!c || !c->has_plan) return set_err(c, COEB_EINVAL, "no batch extracted yet");
    if (d_kps) *d_kps = c->ex.kps.p;
    if (d_desc) *d_desc = c->ex.desc.p;
    if (d_counts) *d_counts = c->ex.counts.p;
    if (kcap) *kcap = c->plan.kcap;
    return COEB_OK;
}

int coeb_extract(coeb_ctx* c, const uint8_t* gray, int W, int H, size_t stride, const coeb_box* boxes, int nbox,
                 const float* tm_xy, int ntm, const int32_t* blur_flag, int nblur, coeb_keypoint* kp_out,
                 uint8_t* desc_out, int cap, int* n_out)
{
    if (!c || !n_out) return set_err(c, COEB_EINVAL, "coeb_extract: invalid arguments");
    *n_out = 0;
    const char* why = "";
    int rc = single_frame_check(gray, W, H, stride, boxes, nbox, tm_xy, ntm, nblur, &why);
    if (rc == 1) return COEB_OK;                            // _image.empty() -> return (:1096-1097)
    if (rc) return set_err(c, rc, why == kWhyNullDynArrays ? std::string("coeb_extract: ") + why : why);
    (void)hipSetDevice(c->device);
    if ((rc = ensure_plan(c, W, H)) || (rc = ensure(c, c->ex.gray_stage, (size_t)W * H))) return rc;
    const int kcap = c->plan.kcap;
    const SingleFrameLayout L = single_frame_layout(W, H, kcap, nbox, ntm);
    if ((rc = pinned(c, L.total))) return rc;
    ExtractBufs b;
    if ((rc = enqueue_single_frame(c, L, gray, W, H, stride, boxes, nbox, tm_xy, ntm, blur_flag, nblur, b))) return rc;
    // with both arrays set, k_out_pack delivers every record the caller can take in the same
    // synchronisation as the count: it copies min(count, guess) records and count <= kcap (kcap
    // sums the levels' out_cap, make_plan), so min(count, cap) <= guess and the second round trip
    // below serves one-array calls only
    const int guess = (kp_out && desc_out) ? std::min(kcap, std::max(cap, 0)) : 0;
    hipStream_t s = main_stream(c);
    hipLaunchKernelGGL(k_out_pack, dim3(16), dim3(256), 0, s, b.counts, static_cast<const uint32_t*>(b.kps),
                       reinterpret_cast<const uint4*>(b.desc), guess, reinterpret_cast<int*>(c->pin_dev + L.o_n),
                       reinterpret_cast<uint32_t*>(c->pin_dev + L.o_k), reinterpret_cast<uint4*>(c->pin_dev + L.o_d));
    HIP_TRY(c, hipGetLastError());
    int n = 0;
    if ((rc = finish_single_frame(c, L, s, &n))) return rc;
    *n_out = n;
    const int m = std::min(n, cap);
    if (m > guess) {                         // one output array only (guess = 0): fetch it by a copy
        if (kp_out)
            HIP_TRY(c, hipMemcpyAsync(c->pin + L.o_k, b.kps, (size_t)m * sizeof(coeb_keypoint), hipMemcpyDeviceToHost, s));
        if (desc_out) HIP_TRY(c, hipMemcpyAsync(c->pin + L.o_d, b.desc, (size_t)m * 32, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
    }
    if (m > 0 && kp_out) memcpy(kp_out, c->pin + L.o_k, (size_t)m * sizeof(coeb_keypoint));
    if (m > 0 && desc_out) memcpy(desc_out, c->pin + L.o_d, (size_t)m * 32);
    if (n > cap) return set_err(c, COEB_ERANGE, "keypoint output capacity too small");
    return COEB_OK;
}

namespace {
// Where k_frame_tail's results and the depth rows it gathers from lie in the page-locked buffer
// (FrameRgbdLayout and RgbdStreamLayout both have these regions).
struct TailRegions { size_t o_n, o_k, o_d, o_kun, o_ur, o_dep, o_depth; };

// k_frame_tail behind the extraction b left on stream s, for coeb_frame_rgbd and coeb_rgbd_stream_frame;
// *guess = the records it packs (frame_rgbd_guess)
int launch_frame_tail(coeb_ctx* c, hipStream_t s, const ExtractBufs& b, const TailRegions& R, int kcap, int cap, bool want_kun,
                      int W, int H, int depth_type, float depth_scale, const coeb_camera* cam, const float dist[5], int* guess)
{
    FrameTail a;
    memset(&a, 0, sizeof(a));
    a.counts = b.counts; a.kps = static_cast<const uint32_t*>(b.kps); a.desc = reinterpret_cast<const uint4*>(b.desc);
    a.guess = *guess = frame_rgbd_guess(kcap, cap);
    a.out_n = reinterpret_cast<int*>(c->pin_dev + R.o_n);
    a.out_k = reinterpret_cast<uint32_t*>(c->pin_dev + R.o_k);
    a.out_d = reinterpret_cast<uint4*>(c->pin_dev + R.o_d);
    a.out_kun = want_kun ? reinterpret_cast<uint32_t*>(c->pin_dev + R.o_kun) : nullptr;
    a.out_ur = reinterpret_cast<float*>(c->pin_dev + R.o_ur);
    a.out_dep = reinterpret_cast<float*>(c->pin_dev + R.o_dep);
    a.depth = c->pin_dev + R.o_depth;
    a.W = W; a.H = H;
    a.depth_u16 = depth_type == COEB_DEPTH_U16;
    a.depth_copy = frame_rgbd_depth_copy(depth_type, depth_scale);
    a.depth_scale = depth_scale;
    a.bf = cam->bf;
    a.undistort = dist && dist[0] != 0.0f;                  // Frame.cc:581-585
    for (int q = 0; q < 12; q++) a.dist.k[q] = (a.undistort && q < 5) ? (double)dist[q] : 0.0;
    a.dist.fx = cam->fx; a.dist.fy = cam->fy; a.dist.cx = cam->cx; a.dist.cy = cam->cy;
    prof_begin(&c->hook, "k_frame_tail", s);
    hipLaunchKernelGGL(k_frame_tail, dim3(16), dim3(256), 0, s, a);
    prof_end(&c->hook, s);
    HIP_TRY(c, hipGetLastError());
    return 0;
}

// the first m records of every output, from the page-locked buffer to the caller's arrays
void frame_tail_copy_out(const coeb_ctx* c, const TailRegions& R, int m, coeb_keypoint* kp, coeb_keypoint* kp_un, uint8_t* desc,
                         float* u_right, float* depth)
{
    if (m <= 0) return;
    memcpy(kp, c->pin + R.o_k, (size_t)m * sizeof(coeb_keypoint));
    memcpy(desc, c->pin + R.o_d, (size_t)m * 32);
    if (kp_un) memcpy(kp_un, c->pin + R.o_kun, (size_t)m * sizeof(coeb_keypoint));
    memcpy(u_right, c->pin + R.o_ur, (size_t)m * 4);
    memcpy(depth, c->pin + R.o_dep, (size_t)m * 4);
}
}  // namespace

int coeb_frame_rgbd(coeb_ctx* c, const uint8_t* gray, int W, int H, size_t stride, const void* depth, size_t depth_stride,
                    int depth_type, float depth_scale, const coeb_camera* cam, const float dist[5], const coeb_box* boxes,
                    int nbox, const float* tm_xy, int ntm, const int32_t* blur_flag, int nblur, coeb_keypoint* kp_out,
                    coeb_keypoint* kp_un_out, uint8_t* desc_out, float* u_right_out, float* depth_out, int cap, int* n_out)
{
    if (!c || !n_out) return set_err(c, COEB_EINVAL, "coeb_frame_rgbd: invalid arguments");
    *n_out = 0;
    const char* why = "";
    int rc = frame_rgbd_check(gray, W, H, stride, depth, depth_stride, depth_type, cam, boxes, nbox, tm_xy, ntm, nblur, kp_out,
                              desc_out, u_right_out, depth_out, &why);
    if (rc == 1) return COEB_OK;                            // _image.empty() -> return (:1096-1097)
    if (rc) return set_err(c, rc, std::string("coeb_frame_rgbd: ") + why);
    (void)hipSetDevice(c->device);
    if ((rc = ensure_plan(c, W, H)) || (rc = ensure(c, c->ex.gray_stage, (size_t)W * H))) return rc;
    const int kcap = c->plan.kcap;
    // the page-locked buffer is sized for the whole call up front: it must not move once the
    // extraction has been enqueued
    const FrameRgbdLayout L = frame_rgbd_layout(W, H, kcap, nbox, ntm, depth_type);
    if ((rc = pinned(c, L.total))) return rc;
    // 1. the gray rows and the extraction, as coeb_extract enqueues them
    ExtractBufs b;
    if ((rc = enqueue_single_frame(c, L, gray, W, H, stride, boxes, nbox, tm_xy, ntm, blur_flag, nblur, b))) return rc;
    hipStream_t s = main_stream(c);
    // 2. while the device extracts, the host packs the depth rows into the buffer (16U as it is:
    // half the bytes, and only the gathered values are ever converted)
    single_frame_stage_rows(c->pin + L.o_depth, depth, H, L.depth_row, depth_stride);
    // 3. the tail kernel behind the extraction
    const TailRegions R{L.o_n, L.o_k, L.o_d, L.o_kun, L.o_ur, L.o_dep, L.o_depth};
    int guess = 0;
    if ((rc = launch_frame_tail(c, s, b, R, kcap, cap, kp_un_out != nullptr, W, H, depth_type, depth_scale, cam, dist, &guess)))
        return rc;
    // 4. the error word, and the call's one synchronisation
    int n = 0;
    if ((rc = finish_single_frame(c, L, s, &n))) return rc;
    *n_out = n;
    // guess = min(kcap, cap) and n <= kcap
    frame_tail_copy_out(c, R, std::min(n, guess), kp_out, kp_un_out, desc_out, u_right_out, depth_out);
    if (n > cap) return set_err(c, COEB_ERANGE, "keypoint output capacity too small");
    return COEB_OK;
}

// ---- the RGB-D Frame constructor on a stream of frames (Frame.cc:157-223) ----
// The object owns one device allocation (coeb_rgbd_stream_host.hpp): two slots that take the frames
// by parity, then the scratch of the corner work and of the LK / fundamental-matrix step; a HIP
// stream for the previous-frame-only work and the two events that order it against the context
// stream.  Nothing of it lies in the context's flow scratch, so other calls on the context and
// other streams leave it alone; what a call shares with them (the page-locked buffer, the stage
// buffer, the extraction's buffers) is free again when the call returns, after its one
// synchronisation.
struct coeb_rgbd_stream {
    coeb_ctx* c = nullptr;
    unsigned flags = 0;
    hipStream_t shadow = nullptr;
    hipEvent_t ev_pyr = nullptr, ev_shadow = nullptr;
    bool shadow_recorded = false;      // ev_shadow marks the end of the corner work enqueued last
    uint8_t* mem = nullptr;
    int w = 0, h = 0;                  // the frame size mem is laid out for
    RgbdStreamSlot slot{};
    size_t o_corner = 0, o_track = 0;
    int prev_w = 0, prev_h = 0;        // the predecessor's size (0: the next frame is a first frame)
    bool corners_due = false;          // no-shadow form: the predecessor's corner work has yet to run
    uint64_t seq = 0;                  // frames taken so far
};

namespace {

StreamFlowFrame stream_frame(const coeb_rgbd_stream* st, int slot)
{
    const RgbdStreamSlot& S = st->slot;
    uint8_t* base = st->mem + (size_t)slot * S.bytes;
    StreamFlowFrame f;
    memset(&f, 0, sizeof(f));
    f.gray = base + S.s_gray;
    for (int l = 1; l < S.L; l++) f.lvl[l] = base + S.s_lvl[l];
    for (int l = 0; l < S.L; l++) f.der[l] = base + S.s_der[l];
    f.pts = reinterpret_cast<float*>(base + S.s_pts);
    f.npts = reinterpret_cast<int*>(base + S.s_npts);
    return f;
}

// the stream's memory laid out for W x H frames (a size change follows a reset: nothing is kept)
int stream_size(coeb_rgbd_stream* st, int W, int H)
{
    coeb_ctx* c = st->c;
    if (st->mem && st->w == W && st->h == H) return 0;
    // the slot is laid out for exactly the levels the flow kernels will walk
    if (stream_flow_levels(W, H) > kStreamLkLevels || stream_flow_levels(W, H) != rgbd_stream_slot(W, H).L)
        return set_err(c, COEB_EINVAL, "coeb_rgbd_stream_frame: image too large");
    if (st->mem) {
        HIP_TRY(c, hipStreamSynchronize(st->shadow));
        int rc = quiesce(c);
        if (rc) return rc;
        if (c->batch_gray >= st->mem && c->batch_gray < st->mem + st->o_track) c->batch_gray = nullptr, c->batch_frames = 0;
        (void)hipFree(st->mem);
        st->mem = nullptr;
    }
    const RgbdStreamSlot S = rgbd_stream_slot(W, H);
    const size_t o_corner = 2 * S.bytes, o_track = o_corner + stream_flow_corner_scratch(W, H);
    const size_t total = o_track + stream_flow_track_scratch();
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&st->mem), total);
    if (e != hipSuccess) {
        st->mem = nullptr;
        return set_err(c, COEB_ENOMEM, std::string("hipMalloc rgbd stream: ") + hipGetErrorString(e));
    }
    st->slot = S; st->o_corner = o_corner; st->o_track = o_track; st->w = W; st->h = H;
    st->shadow_recorded = false;
    return stream_flow_init(c, st->mem + o_corner);
}

}  // namespace

int coeb_rgbd_stream_create(coeb_ctx* c, unsigned flags, coeb_rgbd_stream** out)
{
    if (!c || !out || (flags & ~(unsigned)COEB_STREAM_NO_SHADOW))
        return set_err(c, COEB_EINVAL, "coeb_rgbd_stream_create: invalid arguments");
    *out = nullptr;
    (void)hipSetDevice(c->device);
    coeb_rgbd_stream* st = new coeb_rgbd_stream();
    st->c = c;
    st->flags = flags;
    // the corner work yields to whatever the caller enqueues on the context stream meanwhile
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    if (hipStreamCreateWithPriority(&st->shadow, hipStreamNonBlocking, lo) != hipSuccess ||
        hipEventCreateWithFlags(&st->ev_pyr, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&st->ev_shadow, hipEventDisableTiming) != hipSuccess) {
        const int rc = hip_err(c, hipGetLastError(), "coeb_rgbd_stream_create");
        coeb_rgbd_stream_destroy(st);
        return rc ? rc : COEB_EDEVICE;
    }
    *out = st;
    return COEB_OK;
}

void coeb_rgbd_stream_destroy(coeb_rgbd_stream* st)
{
    if (!st) return;
    coeb_ctx* c = st->c;
    (void)hipSetDevice(c->device);
    if (st->shadow) (void)hipStreamSynchronize(st->shadow);
    if (st->mem) {
        (void)quiesce(c);
        if (c->batch_gray >= st->mem && c->batch_gray < st->mem + st->o_track) c->batch_gray = nullptr, c->batch_frames = 0;
        (void)hipFree(st->mem);
    }
    if (st->ev_pyr) (void)hipEventDestroy(st->ev_pyr);
    if (st->ev_shadow) (void)hipEventDestroy(st->ev_shadow);
    if (st->shadow) (void)hipStreamDestroy(st->shadow);
    delete st;
}

int coeb_rgbd_stream_reset(coeb_rgbd_stream* st)
{
    if (!st) return set_err(nullptr, COEB_EINVAL, "coeb_rgbd_stream_reset: null stream");
    st->prev_w = st->prev_h = 0;
    st->corners_due = false;
    return COEB_OK;
}

int coeb_rgbd_stream_frame(coeb_rgbd_stream* st, const uint8_t* img, size_t img_stride, int channels, int rgb_order, int W,
                           int H, const void* depth, size_t depth_stride, int depth_type, float depth_scale,
                           const coeb_camera* cam, const float dist[5], const coeb_box* boxes, int nbox,
                           coeb_rgbd_stream_out* out)
{
    if (!st) return set_err(nullptr, COEB_EINVAL, "coeb_rgbd_stream_frame: null stream");
    coeb_ctx* c = st->c;
    const char* why = "";
    int rc = rgbd_stream_check(img, img_stride, channels, W, H, depth, depth_stride, depth_type, cam, boxes, nbox, out,
                               st->prev_w, st->prev_h, &why);
    if (rc == 1) {                                          // _image.empty() -> return (:1096-1097)
        out->n = 0; out->n_tm = 0; out->first = st->prev_w == 0;
        return COEB_OK;
    }
    if (rc) return set_err(c, rc, std::string("coeb_rgbd_stream_frame: ") + why);
    (void)hipSetDevice(c->device);
    if ((rc = ensure_plan(c, W, H))) return rc;
    const int kcap = c->plan.kcap;
    const RgbdStreamLayout L = rgbd_stream_layout(W, H, channels, kcap, depth_type);
    // everything that may allocate, before anything is enqueued: the page-locked buffer must not
    // move afterwards, and ensure() drains the context when a buffer grows
    ExtractBufs b;
    if ((rc = pinned(c, L.total)) || (rc = stream_size(st, W, H)) || (rc = extract_bufs(c, 1, b)) ||
        (channels > 1 && (rc = ensure(c, c->ex.stage, L.up_bytes))))
        return rc;
    hipStream_t s = main_stream(c);
    const bool first = st->prev_w == 0;
    const bool shadow = !(st->flags & COEB_STREAM_NO_SHADOW);
    const int cur_slot = rgbd_stream_slot_of(st->seq), prev_slot = cur_slot ^ 1;
    const RgbdStreamSlot& S = st->slot;
    uint8_t* cur_base = st->mem + (size_t)cur_slot * S.bytes;
    const StreamFlowFrame cur = stream_frame(st, cur_slot), prev = stream_frame(st, prev_slot);
    RgbdStreamRes* res = reinterpret_cast<RgbdStreamRes*>(cur_base + S.s_res);
    // 0. the corner work enqueued last has both slots to itself until it ends (after a reset it is
    // the old sequence's: it still writes the slot this frame may take)
    if (st->shadow_recorded) HIP_TRY(c, hipStreamWaitEvent(s, st->ev_shadow, 0));
    st->shadow_recorded = false;
    // 1. the one upload: head + image rows.  A 1-channel frame lands on its slot's head and gray
    // level 0; a colour frame in the stage buffer, from where k_rgbd makes the gray level.
    RgbdStreamHdr* hdr = reinterpret_cast<RgbdStreamHdr*>(c->pin + L.o_hdr);
    memset(hdr, 0, sizeof(*hdr));
    hdr->box_off[1] = nbox;
    if (nbox) memcpy(hdr->box, boxes, (size_t)nbox * sizeof(coeb_box));
    single_frame_stage_rows(c->pin + L.o_img, img, H, L.img_row, img_stride);
    uint8_t* up = channels == 1 ? cur_base + S.s_hdr : c->ex.stage.p;
    HIP_TRY(c, hipMemcpyAsync(up, c->pin, L.up_bytes, hipMemcpyHostToDevice, s));
    const RgbdStreamHdr* dhdr = reinterpret_cast<const RgbdStreamHdr*>(up);
    if (channels > 1 && launch_rgbd_gray(c, up + L.o_img, (int)L.img_row, channels, rgb_order, W, H, cur.gray, s))
        return hip_err(c, hipGetLastError(), "k_rgbd");
    // without a shadow stream the predecessor's corners, subpixel refinement and Scharr planes are
    // made here, in front of the LK step that reads them
    if (!first && st->corners_due && (rc = stream_flow_corners(c, prev, W, H, st->mem + st->o_corner, s))) return rc;
    st->corners_due = false;
    // 2. this frame's LK pyramid; behind it, on the stream's own HIP stream, the work the NEXT call
    // needs of this frame alone
    if ((rc = stream_flow_pyramid(c, cur, W, H, s))) return rc;
    if (shadow) {
        HIP_TRY(c, hipEventRecord(st->ev_pyr, s));
        HIP_TRY(c, hipStreamWaitEvent(st->shadow, st->ev_pyr, 0));
        if ((rc = stream_flow_corners(c, cur, W, H, st->mem + st->o_corner, st->shadow))) return rc;
        HIP_TRY(c, hipEventRecord(st->ev_shadow, st->shadow));
        st->shadow_recorded = true;
    }
    // 3.-5. k_lk against the predecessor, k_fm and the blur flags leave T_M, its count and the flags
    // in the slot's result block, where the extraction reads them
    if (!first) {
        if ((rc = stream_flow_track(c, prev, cur, W, H, st->mem + st->o_track, res->tm, &res->ntm, kStreamTmCap, s))) return rc;
        HIP_TRY(c, hipMemcpyAsync(&res->ncorners, prev.npts, 4, hipMemcpyDeviceToDevice, s));
        if (launch_blur_flags(c, cur.gray, W, H, reinterpret_cast<const float*>(dhdr->box), nbox, res->flag, s))
            return hip_err(c, hipGetLastError(), "k_blur_flags");
        b.tmd = res->tm; b.ntmd = &res->ntm; b.tmd_cap = kStreamTmCap;
    }
    // 6. the extraction (a first frame: no T_M, every flag 0, Frame.cc:205-209)
    if (nbox) {
        b.boxes = reinterpret_cast<const float*>(dhdr->box);
        b.box_off = dhdr->box_off;
        b.blurf = first ? nullptr : res->flag;
    }
    b.gray = cur.gray;
    if (launch_extract(c->plan, c->pl.plan.p, b, 1, s, &c->hook, nullptr)) return hip_err(c, hipGetLastError(), "launch_extract");
    c->batch_frames = 1;
    c->batch_gray = cur.gray;
    // while the device works, the host packs the depth rows the tail kernel gathers from
    single_frame_stage_rows(c->pin + L.o_depth, depth, H, L.depth_row, depth_stride);
    // 7. the tail kernel, as coeb_frame_rgbd launches it
    const TailRegions R{L.o_n, L.o_k, L.o_d, L.o_kun, L.o_ur, L.o_dep, L.o_depth};
    int guess = 0;
    if ((rc = launch_frame_tail(c, s, b, R, kcap, out->cap, out->kp_un != nullptr, W, H, depth_type, depth_scale, cam, dist,
                                &guess)))
        return rc;
    // 8. one copy back -- the gray level the kernels made, when asked for, and the result block
    // behind it -- then the error word and the call's one synchronisation
    const bool gray_back = out->gray && channels > 1;
    if (gray_back || !first) {
        const size_t from = gray_back ? 0 : L.o_res - L.o_gray;
        HIP_TRY(c, hipMemcpyAsync(c->pin + L.o_gray + from, cur_base + S.s_gray + from,
                                  (L.o_res - L.o_gray) - from + (first ? 0 : sizeof(RgbdStreamRes)), hipMemcpyDeviceToHost, s));
    }
    int n = 0;
    SingleFrameLayout LN{};
    LN.o_n = L.o_n;
    rc = finish_single_frame(c, LN, s, &n);
    // the frame is the next call's predecessor whatever is reported below
    st->prev_w = W; st->prev_h = H;
    st->corners_due = !shadow;
    st->seq++;
    if (rc) return rc;
    const RgbdStreamRes* hres = reinterpret_cast<const RgbdStreamRes*>(c->pin + L.o_res);
    if (!first && hres->ncorners < 0)
        return set_err(c, COEB_ERANGE, "coeb_rgbd_stream_frame: the previous frame has more local maxima than the exact selection covers");
    out->first = first;
    out->n_tm = first ? 0 : hres->ntm;
    const int nt = first ? 0 : rgbd_stream_tm_count(hres->ntm, out->tm_cap);
    if (nt > 0) memcpy(out->tm_xy, hres->tm, (size_t)nt * 8);
    for (int i = 0; i < nbox; i++) out->blur_flag[i] = first ? 0 : hres->flag[i];
    if (out->gray) {
        if (channels == 1) {
            for (int y = 0; y < H; y++) memcpy(out->gray + (size_t)y * out->gray_stride, img + (size_t)y * img_stride, (size_t)W);
        } else {
            for (int y = 0; y < H; y++) memcpy(out->gray + (size_t)y * out->gray_stride, c->pin + L.o_gray + (size_t)y * W, (size_t)W);
        }
    }
    out->n = n;
    frame_tail_copy_out(c, R, std::min(n, guess), out->kp, out->kp_un, out->desc, out->u_right, out->depth);
    if (n > out->cap) return set_err(c, COEB_ERANGE, "keypoint output capacity too small");
    return COEB_OK;
}

int coeb_match_lastframe(coeb_ctx* c, const coeb_camera* cam, const coeb_curframe* cur, const coeb_lastframe* last,
                         const float Tcw_cur[16], const float Tcw_last[16], float th, int bmono, int check_ori,
                         int32_t* match_out, int* nmatches)
{
    if (!c || !cam || !cur || !last || !Tcw_cur || !Tcw_last || !nmatches)
        return set_err(c, COEB_EINVAL, "coeb_match_lastframe: invalid arguments");
    *nmatches = 0;
    if (cur->n < 0 || last->n < 0) return set_err(c, COEB_EINVAL, "negative frame size");
    if (cur->n > kCurMax) return set_err(c, COEB_EINVAL, "more than 4095 current keypoints");
    const int n = cur->n, nl = last->n;
    if (n && (!cur->keys_un || !cur->descriptors || !cur->u_right))
        return set_err(c, COEB_EINVAL, "coeb_match_lastframe: missing current-frame arrays");
    if (last_arrays_missing(last)) return set_err(c, COEB_EINVAL, "coeb_match_lastframe: missing LastFrame arrays");
    // the kernel indexes mvScaleFactors[octave] of every LastFrame point with a MapPoint
    for (int i = 0; i < nl; i++)
        if (last->has_mappoint[i] && (last->keys_un[i].octave < 0 || last->keys_un[i].octave >= c->params.nlevels))
            return set_err(c, COEB_EINVAL, "coeb_match_lastframe: LastFrame keypoint octave outside the pyramid");
    if (!match_lastframe_fits(cur->n, nl))
        return set_err(c, COEB_ERANGE, "coeb_match_lastframe: the two frames exceed the LDS budget");
    (void)hipSetDevice(c->device);
    const int cs = std::max(n, 1), ls = std::max(nl, 1);
    int rc;
    SingleFrameBufs& sf = c->sf;
    if ((rc = ensure(c, sf.m_scr, (size_t)ls * kCQ)) || (rc = ensure(c, sf.m_qn, (size_t)ls + kMaxSplit)) ||
        (rc = ensure(c, c->ex.err, 4)))
        return rc;
    hipStream_t s = main_stream(c);
    // every input in one pinned staged copy (ten small pageable copies cost more than the kernel)
    Staged st;
    LastPair lp;
    pack_last_pair(st, cur, last, Tcw_cur, Tcw_last, lp);
    // k_match writes match[cs] and nmatches straight behind the staged inputs (page-locked, no
    // copy back): the region is the inputs alone, and nothing is copied back but the error word
    const size_t o_res = (st.pk.total + 255) & ~(size_t)255;
    const size_t o_err = (o_res + ((size_t)cs + 1) * 4 + 15) & ~(size_t)15;
    if ((rc = pinned(c, o_err + 16)) || (rc = stage_in(c, st.pk, &st.dbase, s))) return rc;
    MatchBufs mb = last_pair_bufs(c, st, lp, cs, ls);
    mb.match = reinterpret_cast<int32_t*>(c->pin_dev + o_res); mb.nmatch = mb.match + cs;
    if (launch_match(make_cam(c, cam), mb, 1, th, bmono, check_ori, 0, s, &c->hook))
        return hip_err(c, hipGetLastError(), "launch_match");
    if ((rc = err_word_async(c, c->pin + o_err))) return rc;
    HIP_TRY(c, hipStreamSynchronize(s));
    if ((rc = err_word_seen(c, c->pin + o_err))) return rc;
    // written by k_match in place
    match_copy_out(reinterpret_cast<const int32_t*>(c->pin + o_res), n, cs, match_out, nmatches);
    return COEB_OK;
}

int coeb_match_localmap(coeb_ctx* c, const coeb_camera* cam, const coeb_curframe* cur, const int32_t* cur_obs,
                        const coeb_localmap* mp, float th, float nnratio, int32_t* match_out, int* nmatches)
{
    if (!c || !cam || !cur || !mp || !nmatches) return set_err(c, COEB_EINVAL, "coeb_match_localmap: invalid arguments");
    *nmatches = 0;
    if (cur->n < 0 || mp->n < 0) return set_err(c, COEB_EINVAL, "negative frame / local map size");
    if (cur->n > kCurMax) return set_err(c, COEB_EINVAL, "more than 4095 current keypoints");
    const int n = cur->n, nq = mp->n;
    if (n && (!cur->keys_un || !cur->descriptors || !cur->u_right))
        return set_err(c, COEB_EINVAL, "coeb_match_localmap: missing current-frame arrays");
    if (nq && (!mp->in_view || !mp->proj_x || !mp->proj_y || !mp->proj_xr || !mp->level || !mp->view_cos ||
               !mp->descriptor || !mp->observations))
        return set_err(c, COEB_EINVAL, "coeb_match_localmap: missing local-map arrays");
    // the kernel indexes mvScaleFactors[level] for every point in view
    for (int q = 0; q < nq; q++)
        if (mp->in_view[q] && (mp->level[q] < 0 || mp->level[q] >= c->tab.nlevels))
            return set_err(c, COEB_EINVAL, "coeb_match_localmap: predicted level outside the pyramid");
    (void)hipSetDevice(c->device);
    const int cs = std::max(n, 1), qs = std::max(nq, 1);
    int rc;
    SingleFrameBufs& sf = c->sf;
    if ((rc = projection_bufs(c, qs))) return rc;
    hipStream_t s = main_stream(c);
    Staged st;
    const CurOff o_c = pack_cur(st, cur);
    const size_t o_co = cur_obs ? st.add(cur_obs, (size_t)n * 4) : st.fill(0xff, (size_t)n * 4);   // -1: all NULL
    const size_t o_v = st.add(mp->in_view, (size_t)nq), o_px = st.add(mp->proj_x, (size_t)nq * 4);
    const size_t o_py = st.add(mp->proj_y, (size_t)nq * 4), o_pxr = st.add(mp->proj_xr, (size_t)nq * 4);
    const size_t o_l = st.add(mp->level, (size_t)nq * 4), o_vc = st.add(mp->view_cos, (size_t)nq * 4);
    const size_t o_qd = st.add(mp->descriptor, (size_t)nq * 32), o_no = st.add(mp->observations, (size_t)nq * 4);
    const size_t o_m = st.take(((size_t)cs + 1) * 4);           // match[cs], nmatch
    if ((rc = st.stage(c, s, true))) return rc;
    LocalBufs b;
    b.cur_kps = st.dev<void>(o_c.k); b.cur_desc = st.dev<uint8_t>(o_c.d); b.cur_ur = st.dev<float>(o_c.ur);
    b.cur_obs = st.dev<int>(o_co); b.cur_n = n;
    b.in_view = st.dev<uint8_t>(o_v); b.proj_x = st.dev<float>(o_px); b.proj_y = st.dev<float>(o_py);
    b.proj_xr = st.dev<float>(o_pxr); b.level = st.dev<int>(o_l); b.view_cos = st.dev<float>(o_vc);
    b.desc = st.dev<uint8_t>(o_qd); b.nobs = st.dev<int>(o_no); b.mp_n = nq;
    b.match = st.dev<int32_t>(o_m); b.nmatch = b.match + cs; b.lists = sf.l_list.p; b.err = c->ex.err.p; b.path = sf.l_path.p;
    rc = launch_match_local(make_cam(c, cam), b, th, nnratio, s, &c->hook);
    if (rc == -2) return set_err(c, COEB_ERANGE, "coeb_match_localmap: frame and local map exceed the LDS budget");
    if (rc) return hip_err(c, hipGetLastError(), "launch_match_local");
    if ((rc = st.finish(c, s, o_m, st.end(), true))) return rc;
    match_copy_out(st.host<int32_t>(o_m), n, cs, match_out, nmatches);
    return COEB_OK;
}

int coeb_match_keyframe(coeb_ctx* c, const coeb_camera* cam, const coeb_curframe* cur, const uint8_t* cur_has,
                        const coeb_keyframe_points* kf, const float Tcw[16], float th, int orb_dist, int check_ori,
                        int32_t* match_out, int* nmatches)
{
    if (!c || !cam || !cur || !kf || !Tcw || !nmatches) return set_err(c, COEB_EINVAL, "coeb_match_keyframe: invalid arguments");
    *nmatches = 0;
    if (cur->n < 0 || kf->n < 0) return set_err(c, COEB_EINVAL, "negative frame / keyframe size");
    if (cur->n > kCurMax) return set_err(c, COEB_EINVAL, "more than 4095 current keypoints");
    const int n = cur->n, nq = kf->n;
    if (n && (!cur->keys_un || !cur->descriptors)) return set_err(c, COEB_EINVAL, "coeb_match_keyframe: missing current-frame arrays");
    if (nq && (!kf->valid || !kf->world_pos || !kf->descriptor || !kf->max_distance || !kf->min_distance || !kf->angle))
        return set_err(c, COEB_EINVAL, "coeb_match_keyframe: missing keyframe arrays");
    if (!match_kf_fits(n, nq)) return set_err(c, COEB_ERANGE, "coeb_match_keyframe: frame and keyframe exceed the LDS budget");
    (void)hipSetDevice(c->device);
    const int cs = std::max(n, 1), qs = std::max(nq, 1);
    int rc;
    SingleFrameBufs& sf = c->sf;
    if ((rc = projection_bufs(c, qs))) return rc;
    hipStream_t s = main_stream(c);
    Staged st;
    const size_t o_k = st.add(cur->keys_un, (size_t)n * sizeof(coeb_keypoint)), o_d = st.add(cur->descriptors, (size_t)n * 32);
    const size_t o_h = cur_has ? st.add(cur_has, (size_t)n) : st.fill(0, (size_t)n);
    const size_t o_v = st.add(kf->valid, (size_t)nq), o_x = st.add(kf->world_pos, (size_t)nq * 12);
    const size_t o_qd = st.add(kf->descriptor, (size_t)nq * 32), o_mx = st.add(kf->max_distance, (size_t)nq * 4);
    const size_t o_mn = st.add(kf->min_distance, (size_t)nq * 4), o_a = st.add(kf->angle, (size_t)nq * 4);
    const size_t o_T = st.add(Tcw, 64);
    const size_t o_m = st.take(((size_t)cs + 1) * 4);           // match[cs], nmatch
    if ((rc = st.stage(c, s, true))) return rc;
    KfBufs b;
    b.cur_kps = st.dev<void>(o_k); b.cur_desc = st.dev<uint8_t>(o_d); b.cur_has = st.dev<uint8_t>(o_h); b.cur_n = n;
    b.valid = st.dev<uint8_t>(o_v); b.xw = st.dev<float>(o_x); b.desc = st.dev<uint8_t>(o_qd);
    b.maxd = st.dev<float>(o_mx); b.mind = st.dev<float>(o_mn); b.angle = st.dev<float>(o_a);
    b.kf_n = nq; b.Tcw = st.dev<float>(o_T);
    b.match = st.dev<int32_t>(o_m); b.nmatch = b.match + cs; b.lists = sf.l_list.p; b.err = c->ex.err.p; b.path = sf.l_path.p;
    rc = launch_match_kf(make_cam(c, cam), b, th, orb_dist, check_ori ? 1 : 0, s, &c->hook);
    if (rc == -2) return set_err(c, COEB_ERANGE, "coeb_match_keyframe: frame and keyframe exceed the LDS budget");
    if (rc) return hip_err(c, hipGetLastError(), "launch_match_kf");
    if ((rc = st.finish(c, s, o_m, st.end(), true))) return rc;
    match_copy_out(st.host<int32_t>(o_m), n, cs, match_out, nmatches);
    return COEB_OK;
}

int coeb_pose_optimization(coeb_ctx* c, const coeb_camera* cam, const coeb_pose_frame* fr, float Tcw[16],
                           uint8_t* outlier_out, int* ninliers)
{
    if (!c || !cam || !fr || !Tcw || !ninliers) return set_err(c, COEB_EINVAL, "coeb_pose_optimization: invalid arguments");
    *ninliers = 0;
    const int n = fr->n;
    if (n < 0) return set_err(c, COEB_EINVAL, "negative frame size");
    if (n && (!fr->has_mappoint || !fr->world_pos || !fr->keys_un || !fr->u_right))
        return set_err(c, COEB_EINVAL, "coeb_pose_optimization: missing frame arrays");
    for (int i = 0; i < n; i++)
        if (fr->has_mappoint[i] && (fr->keys_un[i].octave < 0 || fr->keys_un[i].octave >= c->tab.nlevels))
            return set_err(c, COEB_EINVAL, "coeb_pose_optimization: keypoint octave outside the pyramid");
    (void)hipSetDevice(c->device);
    const int cs = std::max(n, 1);
    int rc;
    if ((rc = pose_scratch(c, cs))) return rc;
    hipStream_t s = main_stream(c);
    // the results first (result, pose, outlier flags: all uploaded, copied back in one go), then the inputs
    Staged st;
    const size_t o_n = st.add(&fr->n, 4), o_res = st.fill(0, 4), o_T = st.add(Tcw, 64), o_out = st.fill(0, (size_t)cs);
    const size_t head = o_out + (size_t)cs;
    const size_t o_h = st.add(fr->has_mappoint, (size_t)n), o_x = st.add(fr->world_pos, (size_t)n * 12);
    const size_t o_k = st.add(fr->keys_un, (size_t)n * sizeof(coeb_keypoint)), o_ur = st.add(fr->u_right, (size_t)n * 4);
    const size_t o_is = st.add(c->tab.inv_sigma2, sizeof(float) * COEB_MAXL);
    if ((rc = st.stage(c, s, false))) return rc;
    const PoseBufs b = pose_bufs(c, st.dev<int>(o_n), st.dev<uint8_t>(o_h), st.dev<float>(o_x), st.dev<void>(o_k),
                                 st.dev<float>(o_ur), st.dev<float>(o_is), st.dev<float>(o_T), st.dev<uint8_t>(o_out),
                                 st.dev<int>(o_res), cs);
    if (launch_pose(b, 1, cam->fx, cam->fy, cam->cx, cam->cy, cam->bf, s, &c->hook))
        return hip_err(c, hipGetLastError(), "launch_pose");
    if ((rc = st.finish(c, s, 0, head, false))) return rc;
    memcpy(Tcw, st.host<float>(o_T), 64);
    if (n && outlier_out)
        for (int i = 0; i < n; i++)
            if (fr->has_mappoint[i]) outlier_out[i] = st.pin[o_out + i];
    *ninliers = *st.host<int>(o_res);
    return COEB_OK;
}

namespace {

// Common body of coeb_search_local_points and coeb_track_local_map (pose: the latter).  Copied back:
// the counts and the pose, matches and outlier flags, and the track fields where asked for.
int track_local_map_impl(coeb_ctx* c, const char* who, bool pose, const coeb_camera* cam, const coeb_curframe* cur,
                         const int32_t* cur_obs, const float* cur_xw, float* Tcw, const coeb_local_points* mp,
                         float cos_limit, float th, float nnratio, int only_tracking, const coeb_track_fields* tf,
                         int32_t* match_out, uint8_t* outlier_out, int* n_to_match, int* nlocal, int* ninliers_pose,
                         int* nmatches_inliers)
{
    const std::string w(who);
    if (!c || !cam || !cur || !Tcw || !mp || !n_to_match || !nlocal || (pose && (!ninliers_pose || !nmatches_inliers)))
        return set_err(c, COEB_EINVAL, w + ": invalid arguments");
    if (cur->n < 0 || mp->n < 0) return set_err(c, COEB_EINVAL, w + ": negative frame / local map size");
    if (cur->n > kCurMax) return set_err(c, COEB_EINVAL, w + ": more than 4095 current keypoints");
    const int n = cur->n, nq = mp->n;
    if (n && (!cur->keys_un || !cur->descriptors || !cur->u_right))
        return set_err(c, COEB_EINVAL, w + ": missing current-frame arrays");
    if (nq && (!mp->valid || !mp->world_pos || !mp->normal || !mp->max_distance || !mp->min_distance || !mp->descriptor ||
               !mp->observations))
        return set_err(c, COEB_EINVAL, w + ": missing local-map arrays");
    if (pose && n && cur_obs && !cur_xw) return set_err(c, COEB_EINVAL, w + ": cur_observations without cur_world_pos");
    // which keypoints take a point is decided on the device: k_pose indexes mvInvLevelSigma2[octave] of any of them
    if (!octaves_in_pyramid(c, cur->keys_un, n)) return set_err(c, COEB_EINVAL, w + ": keypoint octave outside the pyramid");
    // PredictScale's (int)ceil(log(mfMaxDistance / dist) / mfLogScaleFactor) is undefined otherwise
    for (int q = 0; q < nq; q++) {
        if (!mp->valid[q]) continue;
        for (int k = 0; k < 3; k++)
            if (!std::isfinite(mp->world_pos[3 * q + k]) || !std::isfinite(mp->normal[3 * q + k]))
                return set_err(c, COEB_EINVAL, w + ": non-finite position or normal of a valid point");
        const float mn = mp->min_distance[q], mx = mp->max_distance[q];
        if (!(mn > 0.0f && mn <= mx && std::isfinite(mx)))
            return set_err(c, COEB_EINVAL, w + ": distance range of a valid point is not 0 < min <= max < inf");
    }
    if (!match_local_fits(n, nq)) return set_err(c, COEB_ERANGE, w + ": frame and local map exceed the LDS budget");
    (void)hipSetDevice(c->device);
    const int cs = std::max(n, 1), qs = std::max(nq, 1);
    int rc;
    SingleFrameBufs& sf = c->sf;
    if ((rc = ensure(c, sf.l_list, (size_t)qs * kCQ)) || (rc = ensure(c, sf.l_path, 2)) || (rc = ensure(c, c->ex.err, 4)) ||
        (rc = pose_scratch(c, cs)))
        return rc;
    hipStream_t s = main_stream(c);
    Staged st;
    const CurOff o_c = pack_cur(st, cur);
    const size_t o_co = cur_obs ? st.add(cur_obs, (size_t)n * 4) : st.fill(0xff, (size_t)n * 4);   // -1: all NULL
    const size_t nx = pose ? (size_t)n * 12 : 0;    // entry MapPoint positions: the optimiser's only
    const size_t o_cx = cur_obs && cur_xw ? st.add(cur_xw, nx) : st.fill(0, nx);
    const size_t o_v = st.add(mp->valid, (size_t)nq), o_x = st.add(mp->world_pos, (size_t)nq * 12);
    const size_t o_nr = st.add(mp->normal, (size_t)nq * 12), o_mx = st.add(mp->max_distance, (size_t)nq * 4);
    const size_t o_mn = st.add(mp->min_distance, (size_t)nq * 4), o_qd = st.add(mp->descriptor, (size_t)nq * 32);
    const size_t o_no = st.add(mp->observations, (size_t)nq * 4), o_is = st.add(c->tab.inv_sigma2, sizeof(float) * COEB_MAXL);
    const size_t o_T0 = st.add(Tcw, 64);            // the pose the frustum reads
    // results with an initial value: {n, nToMatch, ninliers_pose, mnMatchesInliers}, the pose k_pose updates
    const int32_t cnt[4] = {n, 0, 0, 0};
    const size_t o_cnt = st.add(cnt, 16), o_T = st.add(Tcw, 64);
    // results the kernels write (the track fields only where asked for), then scratch
    const size_t o_m = st.take(((size_t)cs + 1) * 4), o_out = st.take((size_t)cs);
    const size_t head_end = st.end();
    const size_t o_iv = st.take((size_t)qs), o_px = st.take((size_t)qs * 4), o_py = st.take((size_t)qs * 4);
    const size_t o_pxr = st.take((size_t)qs * 4), o_lv = st.take((size_t)qs * 4), o_vc = st.take((size_t)qs * 4);
    const size_t back_end = tf ? st.end() : head_end;
    const size_t o_h2 = st.take((size_t)cs), o_x2 = st.take((size_t)cs * 12), o_o2 = st.take((size_t)cs * 4);
    if ((rc = st.stage(c, s, true))) return rc;
    const MatchCam mcam = make_cam(c, cam);
    LmBufs t;
    memset(&t, 0, sizeof(t));
    int32_t* dcnt = st.dev<int32_t>(o_cnt);
    t.mp_n = nq; t.valid = st.dev<uint8_t>(o_v); t.xw = st.dev<float>(o_x); t.normal = st.dev<float>(o_nr);
    t.maxd = st.dev<float>(o_mx); t.mind = st.dev<float>(o_mn); t.nobs = st.dev<int>(o_no);
    t.Tcw = st.dev<float>(o_T0); t.cos_limit = cos_limit;
    t.in_view = st.dev<uint8_t>(o_iv); t.px = st.dev<float>(o_px); t.py = st.dev<float>(o_py); t.pxr = st.dev<float>(o_pxr);
    t.level = st.dev<int>(o_lv); t.vcos = st.dev<float>(o_vc); t.n_to_match = dcnt + 1;
    t.cur_n = n; t.cur_obs = st.dev<int>(o_co); t.cur_xw = st.dev<float>(o_cx); t.lmatch = st.dev<int>(o_m);
    t.has2 = st.dev<uint8_t>(o_h2); t.xw2 = st.dev<float>(o_x2); t.obs2 = st.dev<int>(o_o2);
    t.outl = st.dev<uint8_t>(o_out); t.only_tracking = only_tracking ? 1 : 0; t.ninl = dcnt + 3;
    if (launch_frustum(mcam, t, s, &c->hook)) return hip_err(c, hipGetLastError(), "launch_frustum");
    LocalBufs b;
    b.cur_kps = st.dev<void>(o_c.k); b.cur_desc = st.dev<uint8_t>(o_c.d); b.cur_ur = st.dev<float>(o_c.ur);
    b.cur_obs = t.cur_obs; b.cur_n = n;
    b.in_view = t.in_view; b.proj_x = t.px; b.proj_y = t.py; b.proj_xr = t.pxr; b.level = t.level; b.view_cos = t.vcos;
    b.desc = st.dev<uint8_t>(o_qd); b.nobs = t.nobs; b.mp_n = nq;
    b.match = st.dev<int>(o_m); b.nmatch = b.match + cs; b.lists = sf.l_list.p; b.err = c->ex.err.p; b.path = sf.l_path.p;
    // nothing in view: the search finds nothing (the reference skips it, Tracking.cc:1261)
    rc = launch_match_local(mcam, b, th, nnratio, s, &c->hook);
    if (rc == -2) return set_err(c, COEB_ERANGE, w + ": frame and local map exceed the LDS budget");
    if (rc) return hip_err(c, hipGetLastError(), "launch_match_local");
    if (pose) {
        if (launch_lm_pose_prep(t, s, &c->hook)) return hip_err(c, hipGetLastError(), "launch_lm_pose_prep");
        const PoseBufs p = pose_bufs(c, dcnt, t.has2, t.xw2, b.cur_kps, b.cur_ur, st.dev<float>(o_is), st.dev<float>(o_T),
                                     st.dev<uint8_t>(o_out), dcnt + 2, cs);
        if (launch_pose(p, 1, cam->fx, cam->fy, cam->cx, cam->cy, cam->bf, s, &c->hook))
            return hip_err(c, hipGetLastError(), "launch_pose");
        if (launch_lm_tail(t, s, &c->hook)) return hip_err(c, hipGetLastError(), "launch_lm_tail");
    }
    if ((rc = st.finish(c, s, o_cnt, back_end, true))) return rc;
    const int32_t* hc = st.host<int32_t>(o_cnt);
    const int32_t* hm = st.host<int32_t>(o_m);
    if (n && match_out) memcpy(match_out, hm, (size_t)n * 4);
    *n_to_match = hc[1];
    *nlocal = hm[cs];
    if (tf && nq) {
        if (tf->in_view) memcpy(tf->in_view, st.pin + o_iv, (size_t)nq);
        if (tf->proj_x) memcpy(tf->proj_x, st.pin + o_px, (size_t)nq * 4);
        if (tf->proj_y) memcpy(tf->proj_y, st.pin + o_py, (size_t)nq * 4);
        if (tf->proj_xr) memcpy(tf->proj_xr, st.pin + o_pxr, (size_t)nq * 4);
        if (tf->level) memcpy(tf->level, st.pin + o_lv, (size_t)nq * 4);
        if (tf->view_cos) memcpy(tf->view_cos, st.pin + o_vc, (size_t)nq * 4);
    }
    if (pose) {
        memcpy(Tcw, st.pin + o_T, 64);
        if (outlier_out)
            for (int i = 0; i < n; i++)
                if (hm[i] >= 0 || (cur_obs && cur_obs[i] >= 0)) outlier_out[i] = st.pin[o_out + i];
        *ninliers_pose = hc[2];
        *nmatches_inliers = hc[3];
    }
    return COEB_OK;
}

}  // namespace

int coeb_search_local_points(coeb_ctx* c, const coeb_camera* cam, const coeb_curframe* cur, const int32_t* cur_obs,
                             const float Tcw[16], const coeb_local_points* points, float cos_limit, float th,
                             float nnratio, const coeb_track_fields* track_fields_out, int32_t* match_out,
                             int* n_to_match, int* nmatches)
{
    return track_local_map_impl(c, "coeb_search_local_points", false, cam, cur, cur_obs, nullptr, const_cast<float*>(Tcw),
                                points, cos_limit, th, nnratio, 0, track_fields_out, match_out, nullptr, n_to_match,
                                nmatches, nullptr, nullptr);
}

int coeb_track_local_map(coeb_ctx* c, const coeb_camera* cam, const coeb_curframe* cur, const int32_t* cur_obs,
                         const float* cur_world_pos, float Tcw[16], const coeb_local_points* points, float cos_limit,
                         float th, float nnratio, int only_tracking, const coeb_track_fields* track_fields_out,
                         int32_t* match_out, uint8_t* outlier_out, int* n_to_match, int* nlocal, int* ninliers_pose,
                         int* nmatches_inliers)
{
    return track_local_map_impl(c, "coeb_track_local_map", true, cam, cur, cur_obs, cur_world_pos, Tcw, points, cos_limit,
                                th, nnratio, only_tracking, track_fields_out, match_out, outlier_out, n_to_match, nlocal,
                                ninliers_pose, nmatches_inliers);
}

// Copied back: the counts and the pose, matches, discards and the transform's ids.
int coeb_track_reference_keyframe(coeb_ctx* c, const coeb_camera* cam, const coeb_curframe* cur,
                                  const int32_t* cur_node_id, int levelsup, const coeb_ref_keyframe* kf, float Tcw[16],
                                  float nnratio, int check_orientation, int min_matches, int32_t* word_out,
                                  int32_t* node_out, double* weight_out, int32_t* match_out, int32_t* discarded_out,
                                  int* nmatches_bow, int* ninliers_pose, int* nmatches, int* nmatches_map)
{
    const std::string w("coeb_track_reference_keyframe");
    if (!c || !cam || !cur || !kf || !Tcw || !nmatches_bow || !ninliers_pose || !nmatches || !nmatches_map)
        return set_err(c, COEB_EINVAL, w + ": invalid arguments");
    const int n = cur->n, nq = kf->bow.n;
    if (n < 0 || nq < 0) return set_err(c, COEB_EINVAL, w + ": negative frame / keyframe size");
    if (n > kCurMax || nq > kCurMax) return set_err(c, COEB_EINVAL, w + ": more than 4095 features");
    const bool transform = !cur_node_id;
    if (transform && levelsup < 0) return set_err(c, COEB_EINVAL, w + ": negative levelsup");
    if (transform && !c->voc.k) return set_err(c, COEB_EINVAL, w + ": no vocabulary (coeb_bow_set_vocabulary)");
    if (n && (!cur->keys_un || !cur->descriptors || !cur->u_right || !match_out))
        return set_err(c, COEB_EINVAL, w + ": missing current-frame arrays");
    if (nq && (!kf->bow.valid || !kf->bow.descriptor || !kf->bow.node_id || !kf->bow.angle || !kf->world_pos ||
               !kf->observations))
        return set_err(c, COEB_EINVAL, w + ": missing keyframe arrays");
    // which keypoints take a point is decided on the device: k_pose indexes mvInvLevelSigma2[octave] of any of them
    if (!octaves_in_pyramid(c, cur->keys_un, n)) return set_err(c, COEB_EINVAL, w + ": keypoint octave outside the pyramid");
    std::vector<float> angle((size_t)n);            // F.mvKeys[i].angle = mvKeysUn[i].angle, contiguous for the matcher
    for (int i = 0; i < n; i++) angle[i] = cur->keys_un[i].angle;
    (void)hipSetDevice(c->device);
    const int cs = std::max(n, 1);
    int rc;
    if ((rc = bow_search_bufs(c, nq, n)) || (rc = pose_scratch(c, cs))) return rc;
    hipStream_t s = main_stream(c);
    Staged st;
    const CurOff o_c = pack_cur(st, cur);
    const size_t o_ca = st.add(angle.data(), (size_t)n * 4), o_cn = transform ? 0 : st.add(cur_node_id, (size_t)n * 4);
    const size_t o_v = st.add(kf->bow.valid, (size_t)nq), o_kd = st.add(kf->bow.descriptor, (size_t)nq * 32);
    const size_t o_kn = st.add(kf->bow.node_id, (size_t)nq * 4), o_ka = st.add(kf->bow.angle, (size_t)nq * 4);
    const size_t o_x = st.add(kf->world_pos, (size_t)nq * 12), o_no = st.add(kf->observations, (size_t)nq * 4);
    const size_t o_is = st.add(c->tab.inv_sigma2, sizeof(float) * COEB_MAXL);
    // results with an initial value: {the optimiser's n, ninliers_pose, nmatches, nmatches_map}, the pose k_pose updates
    const int32_t cnt[4] = {0, 0, 0, 0};
    const size_t o_cnt = st.add(cnt, 16), o_T = st.add(Tcw, 64);
    // results the kernels write (matches, discards, the transform's ids), then scratch
    const size_t o_m = st.take(((size_t)cs + 1) * 4), o_dis = st.take((size_t)cs * 4);
    const size_t o_wd = st.take(transform ? (size_t)cs * 4 : 0), o_nd = st.take(transform ? (size_t)cs * 4 : 0);
    const size_t back_end = st.end();
    const size_t o_has = st.take((size_t)cs), o_xw = st.take((size_t)cs * 12), o_out = st.take((size_t)cs);
    if ((rc = st.stage(c, s, false))) return rc;    // this call does not read the error word
    int32_t* dcnt = st.dev<int32_t>(o_cnt);
    if (transform && n &&
        launch_transform(c, st.dev<uint8_t>(o_c.d), nullptr, n, n, 1, levelsup, st.dev<int>(o_wd), st.dev<int>(o_nd), s))
        return hip_err(c, hipGetLastError(), "k_bow_transform");
    BowSearch bs;
    bs.kf_valid = st.dev<uint8_t>(o_v); bs.kf_desc = st.dev<uint8_t>(o_kd); bs.kf_node = st.dev<int>(o_kn);
    bs.kf_angle = st.dev<float>(o_ka); bs.kf_n = nq;
    bs.cur_desc = st.dev<uint8_t>(o_c.d); bs.cur_node = st.dev<int>(transform ? o_nd : o_cn);
    bs.cur_angle = st.dev<float>(o_ca); bs.cur_n = n; bs.match = st.dev<int>(o_m);
    if (launch_search_by_bow(c, bs, nnratio, check_orientation, s)) return hip_err(c, hipGetLastError(), "launch_search_by_bow");
    TrkBufs t;
    t.cur_n = n; t.match = bs.match; t.nm_bow = bs.match + cs; t.min_matches = min_matches;
    t.kf_xw = st.dev<float>(o_x); t.kf_nobs = st.dev<int>(o_no);
    t.has = st.dev<uint8_t>(o_has); t.xw = st.dev<float>(o_xw); t.pose_n = dcnt; t.outl = st.dev<uint8_t>(o_out);
    t.discarded = st.dev<int>(o_dis); t.nmatches = dcnt + 2; t.nmap = dcnt + 3;
    if (launch_trk_pose_prep(t, s, &c->hook)) return hip_err(c, hipGetLastError(), "launch_trk_pose_prep");
    const PoseBufs p = pose_bufs(c, dcnt, t.has, t.xw, st.dev<void>(o_c.k), st.dev<float>(o_c.ur), st.dev<float>(o_is),
                                 st.dev<float>(o_T), t.outl, dcnt + 1, cs);
    if (launch_pose(p, 1, cam->fx, cam->fy, cam->cx, cam->cy, cam->bf, s, &c->hook))
        return hip_err(c, hipGetLastError(), "launch_pose");
    if (launch_trk_tail(t, s, &c->hook)) return hip_err(c, hipGetLastError(), "launch_trk_tail");
    if ((rc = st.finish(c, s, o_cnt, back_end, false))) return rc;
    const int32_t* hc = st.host<int32_t>(o_cnt);
    const int32_t* hm = st.host<int32_t>(o_m);
    if (transform) {
        const int32_t* h_word = st.host<int32_t>(o_wd);
        if (word_out) memcpy(word_out, h_word, (size_t)n * 4);
        if (node_out) memcpy(node_out, st.pin + o_nd, (size_t)n * 4);
        for (int i = 0; weight_out && i < n; i++) weight_out[i] = word_weight(c, h_word[i]);
    }
    if (n) memcpy(match_out, hm, (size_t)n * 4);
    if (n && discarded_out) memcpy(discarded_out, st.pin + o_dis, (size_t)n * 4);
    memcpy(Tcw, st.pin + o_T, 64);
    *nmatches_bow = hm[cs];
    *ninliers_pose = hc[1];
    *nmatches = hc[2];
    *nmatches_map = hc[3];
    return COEB_OK;
}

// The last frame's MapPoint arrays are among the inputs; k_vo_points updates them in place before
// k_match reads them.  Copied back: the counts and the pose, matches, discards, outlier flags and the
// created points.
static_assert(kVoMaxLast == COEB_VO_MAX_LAST, "k_vo_points' limit is the header's");
int coeb_track_motion_model(coeb_ctx* c, const coeb_camera* cam, const coeb_curframe* cur, const coeb_lastframe* last,
                            const coeb_vo_points* vo, const float Tcw_last[16], float Tcw[16], float th, int bmono,
                            int check_orientation, int min_matches, int32_t* match_out, int32_t* discarded_out,
                            uint8_t* outlier_out, int* nmatches_search, int* ninliers_pose, int* nmatches,
                            int* nmatches_map)
{
    const std::string w("coeb_track_motion_model");
    if (!c || !cam || !cur || !last || !Tcw_last || !Tcw || !nmatches_search || !ninliers_pose || !nmatches || !nmatches_map)
        return set_err(c, COEB_EINVAL, w + ": invalid arguments");
    const int n = cur->n, nl = last->n;
    if (n < 0 || nl < 0) return set_err(c, COEB_EINVAL, w + ": negative frame size");
    if (n > kCurMax) return set_err(c, COEB_EINVAL, w + ": more than 4095 current keypoints");
    if (n && (!cur->keys_un || !cur->descriptors || !cur->u_right || !match_out))
        return set_err(c, COEB_EINVAL, w + ": missing current-frame arrays");
    if (last_arrays_missing(last)) return set_err(c, COEB_EINVAL, w + ": missing LastFrame arrays");
    if (vo && nl && (!vo->depth || !vo->descriptors)) return set_err(c, COEB_EINVAL, w + ": missing visual-odometry arrays");
    if (vo && nl > COEB_VO_MAX_LAST) return set_err(c, COEB_EINVAL, w + ": more LastFrame keypoints than COEB_VO_MAX_LAST");
    if (!match_lastframe_fits(n, nl)) return set_err(c, COEB_ERANGE, w + ": the two frames exceed the LDS budget");
    // which keypoints take a point, and which LastFrame slots get one, is decided on the device: k_pose
    // indexes mvInvLevelSigma2[octave] of the former, k_match mvScaleFactors[octave] of the latter
    if (!octaves_in_pyramid(c, cur->keys_un, n)) return set_err(c, COEB_EINVAL, w + ": keypoint octave outside the pyramid");
    if (!octaves_in_pyramid(c, last->keys_un, nl))
        return set_err(c, COEB_EINVAL, w + ": LastFrame keypoint octave outside the pyramid");
    (void)hipSetDevice(c->device);
    const int cs = std::max(n, 1), ls = std::max(nl, 1);
    const bool run_vo = vo && nl;
    int rc;
    SingleFrameBufs& sf = c->sf;
    if ((rc = ensure(c, sf.m_scr, (size_t)ls * kCQ)) || (rc = ensure(c, sf.m_qn, (size_t)ls + kMaxSplit)) ||
        (rc = ensure(c, c->ex.err, 4)) || (rc = pose_scratch(c, cs)))
        return rc;
    hipStream_t s = main_stream(c);
    Staged st;
    LastPair lp;
    pack_last_pair(st, cur, last, Tcw, Tcw_last, lp);
    const size_t o_vz = run_vo ? st.add(vo->depth, (size_t)nl * 4) : 0, o_vd = run_vo ? st.add(vo->descriptors, (size_t)nl * 32) : 0;
    const size_t o_is = st.add(c->tab.inv_sigma2, sizeof(float) * COEB_MAXL);
    // results with an initial value: {the optimiser's n, ninliers_pose, nmatches, nmatches_map}, the pose k_pose updates
    const int32_t cnt[4] = {0, 0, 0, 0};
    const size_t o_cnt = st.add(cnt, 16), o_T = st.add(Tcw, 64);
    // results the kernels write (matches, discards, outlier flags, the created points), then scratch
    const size_t o_m = st.take(((size_t)cs + 1) * 4), o_dis = st.take((size_t)cs * 4), o_out = st.take((size_t)cs);
    const size_t o_cr = st.take(run_vo ? (size_t)nl : 0), o_cp = st.take(run_vo ? (size_t)nl * 12 : 0);
    const size_t back_end = st.end();
    const size_t o_has = st.take((size_t)cs), o_px = st.take((size_t)cs * 12);
    if ((rc = st.stage(c, s, true))) return rc;
    int32_t* dcnt = st.dev<int32_t>(o_cnt);
    MatchBufs mb = last_pair_bufs(c, st, lp, cs, ls);
    mb.match = st.dev<int>(o_m); mb.nmatch = mb.match + cs;
    if (run_vo) {                                   // the created points replace last-frame slots before k_match reads them
        VoBufs v;
        v.n = nl; v.kps = mb.last_kps; v.depth = st.dev<float>(o_vz); v.desc_in = st.dev<uint8_t>(o_vd);
        v.Tcw_last = mb.Tcw_last; v.th_depth = vo->th_depth;
        v.fx = cam->fx; v.fy = cam->fy; v.cx = cam->cx; v.cy = cam->cy;
        v.has = st.dev<uint8_t>(lp.h); v.xw = st.dev<float>(lp.xw); v.desc = st.dev<uint8_t>(lp.ld); v.nobs = st.dev<int>(lp.nb);
        v.created = st.dev<uint8_t>(o_cr); v.created_pos = st.dev<float>(o_cp);
        if (launch_vo_points(v, s, &c->hook)) return hip_err(c, hipGetLastError(), "launch_vo_points");
    }
    // the 2*th retry below min_matches (:954-958) runs inside k_match
    if (launch_match(make_cam(c, cam), mb, 1, th, bmono, check_orientation, min_matches, s, &c->hook))
        return hip_err(c, hipGetLastError(), "launch_match");
    // the gate (:960) and the gather are TrackReferenceKeyFrame's with the last frame's slots in the
    // KeyFrame's place
    TrkBufs t;
    t.cur_n = n; t.match = mb.match; t.nm_bow = mb.nmatch; t.min_matches = min_matches;
    t.kf_xw = mb.last_xw; t.kf_nobs = mb.last_nobs;
    t.has = st.dev<uint8_t>(o_has); t.xw = st.dev<float>(o_px); t.pose_n = dcnt; t.outl = st.dev<uint8_t>(o_out);
    t.discarded = st.dev<int>(o_dis); t.nmatches = dcnt + 2; t.nmap = dcnt + 3;
    if (launch_trk_pose_prep(t, s, &c->hook)) return hip_err(c, hipGetLastError(), "launch_trk_pose_prep");
    const PoseBufs p = pose_bufs(c, dcnt, t.has, t.xw, mb.cur_kps, mb.cur_ur, st.dev<float>(o_is), st.dev<float>(o_T), t.outl,
                                 dcnt + 1, cs);
    if (launch_pose(p, 1, cam->fx, cam->fy, cam->cx, cam->cy, cam->bf, s, &c->hook))
        return hip_err(c, hipGetLastError(), "launch_pose");
    if (launch_mm_tail(t, s, &c->hook)) return hip_err(c, hipGetLastError(), "launch_mm_tail");
    if ((rc = st.finish(c, s, o_cnt, back_end, true))) return rc;
    const int32_t* hc = st.host<int32_t>(o_cnt);
    const int32_t* hm = st.host<int32_t>(o_m);
    if (n) memcpy(match_out, hm, (size_t)n * 4);
    if (n && discarded_out) memcpy(discarded_out, st.pin + o_dis, (size_t)n * 4);
    if (n && outlier_out) memcpy(outlier_out, st.pin + o_out, (size_t)n);
    if (run_vo) {
        const uint8_t* hcr = st.pin + o_cr;
        if (vo->created_out) memcpy(vo->created_out, hcr, (size_t)nl);
        if (vo->created_pos)
            for (int i = 0; i < nl; i++)
                if (hcr[i]) memcpy(vo->created_pos + 3 * (size_t)i, st.pin + o_cp + 12 * (size_t)i, 12);
    }
    memcpy(Tcw, st.pin + o_T, 64);
    *nmatches_search = hm[cs];
    *ninliers_pose = hc[1];
    *nmatches = hc[2];
    *nmatches_map = hc[3];
    return COEB_OK;
}

// The hypotheses' arrays are staged in rows of one stride per side, cs keypoints / ks KeyFrame points,
// both multiples of 16 so that every row of every element size starts on Pack's 16-byte grid.  Copied
// back: the counts, first_good and the poses, the held indices and the packed outlier flags.
static_assert(COEB_RELOC_MAX_HYP <= 64, "one workgroup per hypothesis, stack arrays below");
int coeb_reloc_refine(coeb_ctx* c, const coeb_camera* cam, const coeb_curframe* cur, coeb_reloc_hypothesis* hyp, int nhyp,
                      float th1, int orb_dist1, float th2, int orb_dist2, int check_orientation, int min_good,
                      int low_good, int enough_good, int32_t* match_out, uint8_t* outlier_out, int32_t* ngood,
                      int32_t* nadditional1, int32_t* nadditional2, int32_t* stage, int* first_good)
{
    const std::string w("coeb_reloc_refine");
    if (!c || !cam || !cur || !hyp || !ngood || !nadditional1 || !nadditional2 || !stage || !first_good)
        return set_err(c, COEB_EINVAL, w + ": invalid arguments");
    if (nhyp < 1 || nhyp > COEB_RELOC_MAX_HYP) return set_err(c, COEB_EINVAL, w + ": nhyp outside 1..COEB_RELOC_MAX_HYP");
    const int n = cur->n, H = nhyp;
    if (n < 0) return set_err(c, COEB_EINVAL, w + ": negative frame size");
    if (n > kCurMax) return set_err(c, COEB_EINVAL, w + ": more than 4095 current keypoints");
    if (n && (!cur->keys_un || !cur->descriptors || !cur->u_right || !match_out))
        return set_err(c, COEB_EINVAL, w + ": missing current-frame arrays");
    int kmax = 0;
    for (int h = 0; h < H; h++) {
        const coeb_keyframe_points& kf = hyp[h].kf;
        if (kf.n < 0) return set_err(c, COEB_EINVAL, w + ": negative keyframe size");
        if (kf.n && (!kf.valid || !kf.world_pos || !kf.descriptor || !kf.max_distance || !kf.min_distance || !kf.angle))
            return set_err(c, COEB_EINVAL, w + ": missing keyframe arrays");
        if (n && (!hyp[h].match || !hyp[h].inlier)) return set_err(c, COEB_EINVAL, w + ": missing match / inlier arrays");
        for (int i = 0; i < n; i++) {
            const int m = hyp[h].match[i];
            if (m < -1 || m >= kf.n) return set_err(c, COEB_EINVAL, w + ": match outside [-1, kf.n)");
            if (hyp[h].inlier[i] && m < 0) return set_err(c, COEB_EINVAL, w + ": an inlier without a match");
        }
        kmax = std::max(kmax, kf.n);
    }
    // which keypoints take a point is decided on the device: k_pose indexes mvInvLevelSigma2[octave] of any of them
    if (!octaves_in_pyramid(c, cur->keys_un, n)) return set_err(c, COEB_EINVAL, w + ": keypoint octave outside the pyramid");
    for (int h = 0; h < H; h++)
        if (!match_kf_fits(n, hyp[h].kf.n)) return set_err(c, COEB_ERANGE, w + ": frame and keyframe exceed the LDS budget");
    if (n == 0) {                                   // no edges, nGood = 0: every hypothesis stops at the first gate
        for (int h = 0; h < H; h++) ngood[h] = nadditional1[h] = nadditional2[h] = stage[h] = 0;
        *first_good = -1;
        return COEB_OK;
    }
    (void)hipSetDevice(c->device);
    const int cs = (n + 15) & ~15, ks = (std::max(kmax, 1) + 15) & ~15;
    int rc;
    const size_t HC = (size_t)H * cs, HK = (size_t)H * ks;
    if ((rc = ensure(c, c->sf.l_list, HK * kCQ)) || (rc = ensure(c, c->ex.err, 4)) || (rc = pose_scratch(c, HC))) return rc;
    hipStream_t s = main_stream(c);
    Staged st;
    // H rows of `stride` elements, row h holding cnt(h) of them (the rest zero)
    auto rows = [&](auto ptr_of, auto cnt_of, size_t stride, size_t elem) {
        const size_t o = st.pk.total;
        for (int h = 0; h < H; h++) {
            const size_t nb = (size_t)cnt_of(h) * elem;
            st.add(nb ? ptr_of(h) : nullptr, nb);
            st.fill(0, stride * elem - ((nb + 15) & ~(size_t)15));
        }
        return o;
    };
    auto all_n = [&](int) { return n; };
    auto kf_n = [&](int h) { return hyp[h].kf.n; };
    int32_t kfn[COEB_RELOC_MAX_HYP], cnt0[4 * COEB_RELOC_MAX_HYP + 4] = {0};
    float T0[16 * COEB_RELOC_MAX_HYP];
    for (int h = 0; h < H; h++) {
        kfn[h] = hyp[h].kf.n;
        memcpy(T0 + 16 * h, hyp[h].Tcw, 64);
    }
    cnt0[4 * H] = H;                                // first_good: none
    const CurOff o_c = pack_cur(st, cur);
    const size_t o_is = st.add(c->tab.inv_sigma2, sizeof(float) * COEB_MAXL), o_kn = st.add(kfn, (size_t)H * 4);
    const size_t o_mi = rows([&](int h) { return (const void*)hyp[h].match; }, all_n, cs, 4);
    const size_t o_in = rows([&](int h) { return (const void*)hyp[h].inlier; }, all_n, cs, 1);
    const size_t o_v = rows([&](int h) { return (const void*)hyp[h].kf.valid; }, kf_n, ks, 1);
    const size_t o_x = rows([&](int h) { return (const void*)hyp[h].kf.world_pos; }, kf_n, ks, 12);
    const size_t o_qd = rows([&](int h) { return (const void*)hyp[h].kf.descriptor; }, kf_n, ks, 32);
    const size_t o_mx = rows([&](int h) { return (const void*)hyp[h].kf.max_distance; }, kf_n, ks, 4);
    const size_t o_mn = rows([&](int h) { return (const void*)hyp[h].kf.min_distance; }, kf_n, ks, 4);
    const size_t o_a = rows([&](int h) { return (const void*)hyp[h].kf.angle; }, kf_n, ks, 4);
    // results with an initial value: {stage, ngood, nadditional1, nadditional2} per hypothesis, first_good, the poses
    const size_t o_cnt = st.add(cnt0, ((size_t)4 * H + 4) * 4), o_T = st.add(T0, (size_t)H * 64);
    // results the kernels write (the held indices, the packed outlier flags), then scratch
    const size_t o_held = st.take(HC * 4), o_oo = st.take(HC);
    const size_t back_end = st.end();
    const size_t o_has = st.take(HC), o_px = st.take(HC * 12), o_out = st.take(HC), o_ao = st.take(HC);
    const size_t o_kh = st.take(HC * sizeof(coeb_keypoint)), o_uh = st.take(HC * 4);
    const size_t o_f = st.take(HK), o_vs = st.take(HK), o_sm = st.take(HC * 4), o_snm = st.take((size_t)H * 4);
    const size_t o_act = st.take((size_t)2 * H), o_pn = st.take((size_t)3 * H * 4), o_pr = st.take((size_t)3 * H * 4);
    const size_t o_path = st.take((size_t)2 * H * 4);
    if ((rc = st.stage(c, s, true))) return rc;
    RrBufs r;
    r.nhyp = H; r.cur_n = n; r.cs = cs; r.ks = ks;
    r.min_good = min_good; r.low_good = low_good; r.enough_good = enough_good;
    r.kps = st.dev<void>(o_c.k); r.ur = st.dev<float>(o_c.ur);
    r.match_in = st.dev<int>(o_mi); r.inlier = st.dev<uint8_t>(o_in);
    r.kf_n = st.dev<int>(o_kn); r.kf_valid = st.dev<uint8_t>(o_v); r.kf_xw = st.dev<float>(o_x);
    r.held = st.dev<int>(o_held); r.has = st.dev<uint8_t>(o_has); r.xw = st.dev<float>(o_px); r.outl = st.dev<uint8_t>(o_out);
    r.at_opt = st.dev<uint8_t>(o_ao); r.kps_h = st.dev<void>(o_kh); r.ur_h = st.dev<float>(o_uh);
    r.found = st.dev<uint8_t>(o_f); r.valid_s = st.dev<uint8_t>(o_vs); r.smatch = st.dev<int>(o_sm); r.snm = st.dev<int>(o_snm);
    r.active = st.dev<uint8_t>(o_act); r.pose_n = st.dev<int>(o_pn); r.pose_res = st.dev<int>(o_pr);
    r.cnt = st.dev<int>(o_cnt); r.first_good = r.cnt + 4 * H; r.outl_out = st.dev<uint8_t>(o_oo);
    const MatchCam mc = make_cam(c, cam);
    auto pose = [&](int k) {                        // the k-th PoseOptimization: F = nhyp, gated by pose_n[k][h] = 0
        const PoseBufs p = pose_bufs(c, r.pose_n + k * H, r.has, r.xw, r.kps_h, r.ur_h, st.dev<float>(o_is), st.dev<float>(o_T),
                                     r.outl, st.dev<int>(o_pr) + k * H, cs);
        return launch_pose(p, H, cam->fx, cam->fy, cam->cx, cam->cy, cam->bf, s, &c->hook);
    };
    auto search = [&](int k, float th, int orb_dist) {
        KfBufs b;
        b.cur_kps = r.kps; b.cur_desc = st.dev<uint8_t>(o_c.d); b.cur_has = r.has; b.cur_n = n;
        b.valid = r.valid_s; b.xw = r.kf_xw; b.desc = st.dev<uint8_t>(o_qd); b.maxd = st.dev<float>(o_mx);
        b.mind = st.dev<float>(o_mn); b.angle = st.dev<float>(o_a); b.kf_n = kmax;
        b.Tcw = st.dev<float>(o_T); b.match = st.dev<int>(o_sm); b.nmatch = st.dev<int>(o_snm);
        b.lists = c->sf.l_list.p; b.err = c->ex.err.p; b.path = st.dev<int>(o_path);
        b.kf_n_arr = r.kf_n; b.active = r.active + k * H; b.cur_stride = cs; b.kf_stride = ks; b.npairs = H;
        return launch_match_kf(mc, b, th, orb_dist, check_orientation ? 1 : 0, s, &c->hook);
    };
    if (launch_rr_enter(r, s, &c->hook) || pose(0) || launch_rr_after1(r, s, &c->hook) || search(0, th1, orb_dist1) ||
        launch_rr_merge(r, 1, s, &c->hook) || pose(1) || launch_rr_after2(r, s, &c->hook) || search(1, th2, orb_dist2) ||
        launch_rr_merge(r, 2, s, &c->hook) || pose(2) || launch_rr_tail(r, s, &c->hook))
        return hip_err(c, hipGetLastError(), "coeb_reloc_refine launch");
    if ((rc = st.finish(c, s, o_cnt, back_end, true))) return rc;
    const int32_t* hc = st.host<int32_t>(o_cnt);
    for (int h = 0; h < H; h++) {
        stage[h] = hc[4 * h]; ngood[h] = hc[4 * h + 1]; nadditional1[h] = hc[4 * h + 2]; nadditional2[h] = hc[4 * h + 3];
        memcpy(hyp[h].Tcw, st.pin + o_T + (size_t)h * 64, 64);
        memcpy(match_out + (size_t)h * n, st.pin + o_held + (size_t)h * cs * 4, (size_t)n * 4);
        if (outlier_out) {                          // written where the keypoint held a point at the last optimisation run
            const uint8_t* fl = st.pin + o_oo + (size_t)h * cs;
            for (int i = 0; i < n; i++)
                if (fl[i] != 2) outlier_out[(size_t)h * n + i] = fl[i];
        }
    }
    *first_good = hc[4 * H] < H ? hc[4 * H] : -1;
    return COEB_OK;
}

namespace {

// Common body of the batch matchers.  dT_cur: device poses, pair p (current frame p+1) at
// dT_cur + 16 p; LastFrame poses are identities (frame p is the world frame of its pair).
int match_batch_impl(coeb_ctx* c, const float* d_depth, int F, int W, int H, const coeb_camera* cam,
                     const float* dT_cur, float th, int32_t nobs, bool wait_main)
{
    const int K = c->plan.kcap;
    if (K > kCurMax) return set_err(c, COEB_EINVAL, "keypoint capacity exceeds the matcher limit (4095)");
    int rc;
    BatchMatchBufs& bm = c->bm;
    const int qs = K + kMaxSplit;                           // split-list counts + kMaxSplit flags per pair (last_stride = K)
    if ((rc = ensure(c, bm.b_mqn, (size_t)F * qs)) || (rc = ensure(c, bm.b_ur, (size_t)F * K)) || (rc = ensure(c, bm.b_dep, (size_t)F * K)) ||
        (rc = ensure(c, bm.b_xw, (size_t)F * K * 3)) || (rc = ensure(c, bm.b_has, (size_t)F * K)) ||
        (rc = ensure(c, bm.b_outl, (size_t)F * K)) || (rc = ensure(c, bm.b_nobs, (size_t)F * K)) ||
        (rc = ensure(c, bm.b_match, (size_t)F * K)) || (rc = ensure(c, bm.b_nm, (size_t)F)) ||
        (rc = ensure(c, bm.b_scr, (size_t)F * K * kCQ)) || (rc = ensure(c, c->ex.err, 4)))
        return rc;
    if (c->ident_frames < F || !bm.b_I.p) {
        const int n = std::max(F, c->max_batch);
        HIP_TRY(c, hipStreamSynchronize(main_stream(c)));
        if ((rc = ensure(c, bm.b_I, (size_t)n * 16))) return rc;
        std::vector<float> I((size_t)n * 16, 0.f);
        for (int p = 0; p < n; p++) I[(size_t)p * 16 + 0] = I[(size_t)p * 16 + 5] = I[(size_t)p * 16 + 10] = I[(size_t)p * 16 + 15] = 1.f;
        HIP_TRY(c, hipMemcpy(bm.b_I.p, I.data(), I.size() * 4, hipMemcpyHostToDevice));
        c->ident_frames = n;
    }
    float *ur = bm.b_ur.p, *xw = bm.b_xw.p;
    uint8_t *has = bm.b_has.p, *outl = bm.b_outl.p, *desc = c->ex.desc.p;
    int32_t *nobsb = bm.b_nobs.p, *counts = c->ex.counts.p;
    const coeb_keypoint* kps = c->ex.kps.p;
    const MatchCam mcam = make_cam(c, cam);
    // chunk k (frames [f0, f1)) on its stream: prep, then the pairs whose current frame is in
    // the chunk; the first of them needs chunk k-1's last frame prepared
    const bool chunked = c->extract_chunked && (int)c->chunk.size() > 2 && c->chunk.back() == F;
    const int n = chunked ? (int)c->chunk.size() - 1 : 1;
    if (!chunked) main_stream(c);
    else if (wait_main) HIP_TRY(c, hipEventRecord(c->ev_main, c->stream));
    for (int k = 0; k < n; k++) {
        const int f0 = chunked ? c->chunk[k] : 0, f1 = chunked ? c->chunk[k + 1] : F;
        hipStream_t s = chunked ? c->subs[k] : main_stream(c);
        if (chunked && wait_main) HIP_TRY(c, hipStreamWaitEvent(s, c->ev_main, 0));
        PrepBufs pb;
        memset(&pb, 0, sizeof(pb));
        const int64_t o = (int64_t)f0 * K;
        pb.kps = kps + o; pb.n = counts + f0; pb.stride = K; pb.depth = d_depth + (int64_t)f0 * W * H; pb.W = W; pb.H = H;
        pb.bf = cam->bf; pb.fx = cam->fx; pb.fy = cam->fy; pb.cx = cam->cx; pb.cy = cam->cy;
        pb.ur = ur + o; pb.dep = bm.b_dep.p + o; pb.has = has + o; pb.outl = outl + o; pb.xw = xw + 3 * o;
        pb.nobs = nobsb + o; pb.nobs_value = nobs;
        if (launch_prep(pb, f1 - f0, s, &c->hook)) return hip_err(c, hipGetLastError(), "launch_prep");
        if (chunked) {
            HIP_TRY(c, hipEventRecord(c->ev_prep[k], s));
            if (k > 0) HIP_TRY(c, hipStreamWaitEvent(s, c->ev_prep[k - 1], 0));
        }
        const int p0 = std::max(f0, 1) - 1, np = f1 - std::max(f0, 1);   // pair p: current p+1, last p
        if (np > 0) {
            const int64_t q = (int64_t)p0 * K;
            MatchBufs mb;
            memset(&mb, 0, sizeof(mb));
            mb.cur_kps = kps + q + K; mb.cur_desc = desc + (q + K) * 32; mb.cur_n = counts + p0 + 1; mb.cur_ur = ur + q + K;
            mb.cur_stride = K;
            mb.last_kps = kps + q; mb.last_desc = desc + q * 32; mb.last_n = counts + p0; mb.last_has = has + q;
            mb.last_out = outl + q; mb.last_xw = xw + 3 * q; mb.last_nobs = nobsb + q; mb.last_stride = K;
            mb.Tcw_cur = dT_cur + 16 * p0; mb.Tcw_last = bm.b_I.p + 16 * p0;
            mb.match = bm.b_match.p + q + K; mb.nmatch = bm.b_nm.p + p0 + 1; mb.scratch = bm.b_scr.p + q * kCQ;
            mb.scratch_stride = K * kCQ; mb.err = c->ex.err.p;
            mb.qn = bm.b_mqn.p + (int64_t)p0 * qs; mb.qn_stride = qs;
            if (COEB_MATCH_CLOCK) {
                if ((rc = ensure(c, c->tim.m_timing, (size_t)F * 16))) return rc;
                mb.timing = c->tim.m_timing.p + (int64_t)p0 * 16;
            }
            if (launch_match(mcam, mb, np, th, 0, 1, 20, s, &c->hook)) return hip_err(c, hipGetLastError(), "launch_match");
        }
        if (chunked) HIP_TRY(c, hipEventRecord(c->ev_mdone[k], s));
    }
    c->mdone_valid = chunked;
    if (chunked) c->pending_join = true;
    c->batch_nobs = nobs;
    return COEB_OK;
}

int match_batch_check(coeb_ctx* c, const float* d_depth, int F, int W, int H, const coeb_camera* cam, const float* T)
{
    if (!c || !d_depth || !cam || !T || F <= 0) return set_err(c, COEB_EINVAL, "coeb_match_batch_device: invalid arguments");
    if (!c->has_plan || c->batch_frames != F || c->plan.W != W || c->plan.H != H)
        return set_err(c, COEB_EINVAL, "coeb_match_batch_device: must follow coeb_extract_batch_device on the same batch");
    return COEB_OK;
}

}  // namespace

int coeb_match_batch_device(coeb_ctx* c, const float* d_depth, int F, int W, int H, const coeb_camera* cam,
                            const float* Tcw, float th, int32_t nobs)
{
    int rc;
    if ((rc = match_batch_check(c, d_depth, F, W, H, cam, Tcw))) return rc;
    (void)hipSetDevice(c->device);
    if ((rc = ensure(c, c->bm.b_T, (size_t)F * 16))) return rc;
    float* dT = c->bm.b_T.p;
    // the previous batch's matchers may still read b_T: join them before overwriting it
    HIP_TRY(c, hipMemcpyAsync(dT, Tcw, (size_t)F * 64, hipMemcpyHostToDevice, main_stream(c)));
    return match_batch_impl(c, d_depth, F, W, H, cam, dT + 16, th, nobs, true);
}

int coeb_match_batch_device_tcw(coeb_ctx* c, const float* d_depth, int F, int W, int H, const coeb_camera* cam,
                                const float* d_Tcw, float th, int32_t nobs)
{
    int rc;
    if ((rc = match_batch_check(c, d_depth, F, W, H, cam, d_Tcw))) return rc;
    (void)hipSetDevice(c->device);
    return match_batch_impl(c, d_depth, F, W, H, cam, d_Tcw + 16, th, nobs, false);
}

int coeb_batch_match_results(coeb_ctx* c, const int32_t** d_match, const int32_t** d_nmatches)
{
    if (!c) return COEB_EINVAL;
    if (d_match) *d_match = c->bm.b_match.p;
    if (d_nmatches) *d_nmatches = c->bm.b_nm.p;
    return COEB_OK;
}

int coeb_pose_batch_device(coeb_ctx* c, const coeb_camera* cam, int F, const float* d_Tcw, int32_t min_matches)
{
    if (!c || !cam || !d_Tcw || F <= 0) return set_err(c, COEB_EINVAL, "coeb_pose_batch_device: invalid arguments");
    if (!c->has_plan || c->batch_frames != F || !c->bm.b_match.p || !c->bm.b_xw.p)
        return set_err(c, COEB_EINVAL, "coeb_pose_batch_device: must follow coeb_match_batch_device on the same batch");
    (void)hipSetDevice(c->device);
    const int K = c->plan.kcap;
    int rc;
    BatchPoseBufs& bp = c->bp;
    if ((rc = ensure(c, bp.t_T, (size_t)F * 16)) || (rc = ensure(c, bp.t_xw, (size_t)F * K * 3)) ||
        (rc = ensure(c, bp.t_isg, COEB_MAXL)) || (rc = ensure(c, bp.t_has, (size_t)F * K)) ||
        (rc = ensure(c, bp.t_outl, (size_t)F * K)) || (rc = ensure(c, bp.t_act, (size_t)F * K)) ||
        (rc = ensure(c, bp.t_n, (size_t)F)) || (rc = ensure(c, bp.t_res, (size_t)F)) ||
        (rc = ensure(c, bp.t_edge, (size_t)F * K)) || (rc = ensure(c, bp.t_chi, (size_t)F * K)) ||
        (rc = ensure(c, bp.t_kp, (size_t)F * K)) || (rc = ensure(c, bp.t_ur, (size_t)F * K)))
        return rc;
    hipStream_t s = main_stream(c);                 // joins the matchers' chunk streams
    if (!c->pose_stream) {
        HIP_TRY(c, hipStreamCreateWithFlags(&c->pose_stream, hipStreamNonBlocking));
        HIP_TRY(c, hipEventCreateWithFlags(&c->ev_tprep, hipEventDisableTiming));
        HIP_TRY(c, hipEventCreateWithFlags(&c->ev_pose, hipEventDisableTiming));
    }
    join_pose(c);                                   // the previous batch's k_pose still reads t_*
    HIP_TRY(c, hipMemsetAsync(bp.t_has.p, 0, (size_t)F * K, s));
    HIP_TRY(c, hipMemsetAsync(bp.t_outl.p, 0, (size_t)F * K, s));
    HIP_TRY(c, hipMemsetAsync(bp.t_res.p, 0, (size_t)F * 4, s));
    TrackPrepBufs t;
    memset(&t, 0, sizeof(t));
    t.match = c->bm.b_match.p; t.nmatch = c->bm.b_nm.p; t.counts = c->ex.counts.p; t.last_xw = c->bm.b_xw.p;
    t.kps_in = c->ex.kps.p; t.ur_in = c->bm.b_ur.p;
    t.kps_out = bp.t_kp.p; t.ur_out = bp.t_ur.p;
    t.Tin = d_Tcw; t.Tout = bp.t_T.p; t.has = bp.t_has.p; t.xw = bp.t_xw.p; t.n = bp.t_n.p; t.isg_out = bp.t_isg.p;
    for (int l = 0; l < COEB_MAXL; l++) t.isg[l] = l < c->tab.nlevels ? c->tab.inv_sigma2[l] : 0.f;
    t.stride = K;
    t.min_matches = min_matches;
    if (launch_track_prep(t, F, s, &c->hook)) return hip_err(c, hipGetLastError(), "launch_track_prep");
    if (F < 2) return COEB_OK;
    const int64_t o = K;                            // frame 1 = current frame of pair 0
    PoseBufs b;
    b.n = bp.t_n.p + 1; b.has_mp = bp.t_has.p + o; b.xw = bp.t_xw.p + 3 * o;
    b.kps = bp.t_kp.p + o; b.ur = bp.t_ur.p + o;
    b.inv_sigma2 = bp.t_isg.p; b.Tcw = bp.t_T.p + 16; b.outlier = bp.t_outl.p + o; b.result = bp.t_res.p + 1;
    b.edges = bp.t_edge.p + o; b.active = bp.t_act.p + o; b.chi2 = bp.t_chi.p + o; b.stride = K;
    b.timing = nullptr;
    if (COEB_POSE_CLOCK) {                                   // diagnostic phase clocks, tools/_pose_timing.py
        if ((rc = ensure(c, c->tim.p_timing, (size_t)F * 8))) return rc;
        long long* tmb = c->tim.p_timing.p;
        HIP_TRY(c, hipMemsetAsync(tmb, 0, (size_t)F * 64, s));
        b.timing = tmb + 8;
    }
    HIP_TRY(c, hipEventRecord(c->ev_tprep, s));
    HIP_TRY(c, hipStreamWaitEvent(c->pose_stream, c->ev_tprep, 0));
    if (launch_pose(b, F - 1, cam->fx, cam->fy, cam->cx, cam->cy, cam->bf, c->pose_stream, &c->hook))
        return hip_err(c, hipGetLastError(), "launch_pose");
    HIP_TRY(c, hipEventRecord(c->ev_pose, c->pose_stream));
    c->pose_pending = true;
    c->pose_frames = F;
    c->pose_min_matches = min_matches;
    c->tlm_frames = 0;
    return COEB_OK;
}

int coeb_batch_pose_results(coeb_ctx* c, const float** d_Tcw, const int32_t** d_ninliers, const uint8_t** d_outlier)
{
    if (!c || !c->bp.t_T.p) return set_err(c, COEB_EINVAL, "coeb_batch_pose_results: no batch pose yet");
    join_pose(c);
    if (d_Tcw) *d_Tcw = c->bp.t_T.p;
    if (d_ninliers) *d_ninliers = c->bp.t_res.p;
    if (d_outlier) *d_outlier = c->bp.t_outl.p;
    return COEB_OK;
}

int coeb_track_local_map_batch_device(coeb_ctx* c, const coeb_camera* cam, int F, int32_t nkf, float th, float nnratio)
{
    if (!c || !cam || F <= 0 || nkf < 1 || nkf > 2 || !(th > 0) || !(nnratio > 0))
        return set_err(c, COEB_EINVAL, "coeb_track_local_map_batch_device: invalid arguments");
    if (!c->has_plan || c->batch_frames != F || c->pose_frames != F || !c->bp.t_T.p)
        return set_err(c, COEB_EINVAL, "coeb_track_local_map_batch_device: must follow coeb_pose_batch_device on the same batch");
    if (c->tlm_frames) return set_err(c, COEB_EINVAL, "coeb_track_local_map_batch_device: already run on this batch");
    (void)hipSetDevice(c->device);
    const int K = c->plan.kcap;
    const int64_t FK = (int64_t)F * K, FM = 2 * FK;
    int rc;
    TlmBufs t;
    memset(&t, 0, sizeof(t));
    TrackLocalMapBufs& tl = c->tl;
    const BatchPoseBufs& bp = c->bp;
    if ((rc = ensure(c, tl.tl_sdesc, (size_t)(FK + K) * 32)) || (rc = ensure(c, tl.tl_soct, (size_t)FK)) ||
        (rc = ensure(c, tl.tl_shas, (size_t)FK)) || (rc = ensure(c, tl.tl_sxw, (size_t)FK * 3)) ||
        (rc = ensure(c, tl.tl_sm1, (size_t)FK)) || (rc = ensure(c, tl.tl_scnt, (size_t)F)) ||
        (rc = ensure(c, tl.tl_snm1, (size_t)F)) || (rc = ensure(c, tl.tl_seen, (size_t)FK)) ||
        (rc = ensure(c, tl.tl_cobs, (size_t)FK)) || (rc = ensure(c, tl.tl_nmap, (size_t)F)) ||
        (rc = ensure(c, tl.tl_active, (size_t)F)) || (rc = ensure(c, tl.tl_inview, (size_t)FM)) ||
        (rc = ensure(c, tl.tl_px, (size_t)FM)) || (rc = ensure(c, tl.tl_py, (size_t)FM)) ||
        (rc = ensure(c, tl.tl_pxr, (size_t)FM)) || (rc = ensure(c, tl.tl_level, (size_t)FM)) ||
        (rc = ensure(c, tl.tl_vcos, (size_t)FM)) || (rc = ensure(c, tl.tl_lnobs, (size_t)FM)) ||
        (rc = ensure(c, tl.tl_lxw, (size_t)FM * 3)) || (rc = ensure(c, tl.tl_lmatch, (size_t)FK)) ||
        (rc = ensure(c, tl.tl_nlocal, (size_t)F)) || (rc = ensure(c, tl.tl_path, (size_t)F * 2)) ||
        (rc = ensure(c, tl.tl_lists, (size_t)FM * kCQ)) ||
        (rc = ensure(c, tl.tl_has2, (size_t)FK)) || (rc = ensure(c, tl.tl_xw2, (size_t)FK * 3)) ||
        (rc = ensure(c, tl.tl_T2, (size_t)F * 16)) || (rc = ensure(c, tl.tl_outl2, (size_t)FK)) ||
        (rc = ensure(c, tl.tl_n2, (size_t)F)) || (rc = ensure(c, tl.tl_res2, (size_t)F)) ||
        (rc = ensure(c, c->ex.err, 4)))
        return rc;
    uint8_t *s_desc = tl.tl_sdesc.p, *act = tl.tl_active.p, *inv = tl.tl_inview.p, *has2 = tl.tl_has2.p, *outl2 = tl.tl_outl2.p;
    float *px = tl.tl_px.p, *py = tl.tl_py.p, *pxr = tl.tl_pxr.p, *vc = tl.tl_vcos.p, *xw2 = tl.tl_xw2.p, *T2 = tl.tl_T2.p;
    int32_t *s_cnt = tl.tl_scnt.p, *cobs = tl.tl_cobs.p, *lvl = tl.tl_level.p, *lno = tl.tl_lnobs.p, *lmatch = tl.tl_lmatch.p,
            *n2 = tl.tl_n2.p;
    t.K = K; t.nkf = nkf; t.nobs = c->batch_nobs; t.min_matches = c->pose_min_matches; t.min_map = 10;
    t.kps = c->ex.kps.p; t.desc = c->ex.desc.p; t.counts = c->ex.counts.p;
    t.match1 = c->bm.b_match.p; t.nmatch1 = c->bm.b_nm.p; t.has = c->bm.b_has.p; t.xw = c->bm.b_xw.p;
    t.s_desc = s_desc; t.s_oct = tl.tl_soct.p; t.s_has = tl.tl_shas.p; t.s_xw = tl.tl_sxw.p; t.s_m1 = tl.tl_sm1.p;
    t.s_cnt = s_cnt; t.s_nm1 = tl.tl_snm1.p;
    t.T1 = bp.t_T.p; t.has1 = bp.t_has.p; t.outl1 = bp.t_outl.p; t.xw1 = bp.t_xw.p;
    t.seen = tl.tl_seen.p; t.cur_obs = cobs; t.nmap = tl.tl_nmap.p; t.active = act;
    t.in_view = inv; t.px = px; t.py = py; t.pxr = pxr; t.level = lvl; t.vcos = vc; t.lm_nobs = lno; t.lm_xw = tl.tl_lxw.p;
    t.lmatch = lmatch; t.has2 = has2; t.xw2 = xw2; t.T2 = T2; t.outl2 = outl2; t.n2 = n2;
    // the snapshot runs on the context stream, after this batch's matcher and before the next
    // batch's extraction; coeb_pose_batch_device already joined the previous pose-stream work
    hipStream_t s = main_stream(c);
    if (launch_tlm_snapshot(t, F, s, &c->hook)) return hip_err(c, hipGetLastError(), "launch_tlm_snapshot");
    if (F < 2) { c->tlm_frames = F; return COEB_OK; }
    if (!c->ev_tlm) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_tlm, hipEventDisableTiming));
    HIP_TRY(c, hipEventRecord(c->ev_tlm, s));
    hipStream_t ps = c->pose_stream;                // after the first k_pose
    HIP_TRY(c, hipStreamWaitEvent(ps, c->ev_tlm, 0));
    const MatchCam mcam = make_cam(c, cam);
    if (launch_tlm_frustum(mcam, t, F, ps, &c->hook)) return hip_err(c, hipGetLastError(), "launch_tlm_frustum");
    LocalBufs lb;
    lb.cur_kps = bp.t_kp.p + K;
    lb.cur_desc = s_desc + (int64_t)2 * K * 32;      // frame 1 = row 2
    lb.cur_ur = bp.t_ur.p + K;
    lb.cur_obs = cobs + K; lb.cur_n = K;
    const int64_t M = 2 * (int64_t)K;
    lb.in_view = inv + M; lb.proj_x = px + M; lb.proj_y = py + M; lb.proj_xr = pxr + M; lb.level = lvl + M;
    lb.view_cos = vc + M; lb.nobs = lno + M; lb.mp_n = (int)M;
    lb.desc = s_desc;                                // frame 1's local map: KF2 = frame -1 (row 0), KF1 = frame 0
    lb.match = lmatch + K; lb.nmatch = tl.tl_nlocal.p + 1; lb.lists = tl.tl_lists.p; lb.err = c->ex.err.p;
    lb.path = tl.tl_path.p + 2;
    lb.cur_n_arr = s_cnt + 1; lb.active = act + 1; lb.npairs = F - 1; lb.cur_stride = K; lb.mp_stride = (int)M;
    lb.mp_desc_stride = K;
    rc = launch_match_local(mcam, lb, th, nnratio, ps, &c->hook);
    if (rc == -2) return set_err(c, COEB_ERANGE, "coeb_track_local_map_batch_device: frame and local map exceed the LDS budget");
    if (rc) return hip_err(c, hipGetLastError(), "launch_match_local");
    if (launch_tlm_pose_prep(t, F, ps, &c->hook)) return hip_err(c, hipGetLastError(), "launch_tlm_pose_prep");
    PoseBufs b;
    const int64_t o = K;
    b.n = n2 + 1; b.has_mp = has2 + o; b.xw = xw2 + 3 * o;
    b.kps = bp.t_kp.p + o; b.ur = bp.t_ur.p + o;
    b.inv_sigma2 = bp.t_isg.p; b.Tcw = T2 + 16; b.outlier = outl2 + o; b.result = tl.tl_res2.p + 1;
    b.edges = bp.t_edge.p + o; b.active = bp.t_act.p + o; b.chi2 = bp.t_chi.p + o; b.stride = K; b.timing = nullptr;
    if (launch_pose(b, F - 1, cam->fx, cam->fy, cam->cx, cam->cy, cam->bf, ps, &c->hook))
        return hip_err(c, hipGetLastError(), "launch_pose");
    HIP_TRY(c, hipEventRecord(c->ev_pose, ps));
    c->pose_pending = true;
    c->tlm_frames = F;
    return COEB_OK;
}

int coeb_batch_track_results(coeb_ctx* c, const float** d_Tcw, const int32_t** d_ninliers, const int32_t** d_nmatches_map,
                             const int32_t** d_nlocal, const int32_t** d_local_match, const uint8_t** d_outlier)
{
    if (!c || !c->tlm_frames) return set_err(c, COEB_EINVAL, "coeb_batch_track_results: no batch TrackLocalMap yet");
    join_pose(c);
    if (d_Tcw) *d_Tcw = c->tl.tl_T2.p;
    if (d_ninliers) *d_ninliers = c->tl.tl_res2.p;
    if (d_nmatches_map) *d_nmatches_map = c->tl.tl_nmap.p;
    if (d_nlocal) *d_nlocal = c->tl.tl_nlocal.p;
    if (d_local_match) *d_local_match = c->tl.tl_lmatch.p;
    if (d_outlier) *d_outlier = c->tl.tl_outl2.p;
    return COEB_OK;
}

int coeb_stereo_from_rgbd(coeb_ctx* c, const coeb_keypoint* kps, int n, const float* depth, int W, int H,
                          size_t dstride, float bf, float* ur_out, float* dep_out)
{
    if (!c || (n > 0 && (!kps || !depth || !ur_out || !dep_out)) || n < 0 || dstride < (size_t)W)
        return set_err(c, COEB_EINVAL, "coeb_stereo_from_rgbd: invalid arguments");
    if (n == 0) return COEB_OK;
    (void)hipSetDevice(c->device);
    int rc;
    hipStream_t s = main_stream(c);
    // everything through the context's page-locked buffer, addressed by k_prep in place: the
    // keypoints and their count in, the depth rows (it touches ~n of the W*H values, so copying
    // the whole map to the device -- 1.2 MB at 640x480 -- would cost more than the lookups), and
    // uR / depth written straight back; one launch and one synchronisation, no copy operations
    const size_t o_n = 0, o_k = 256, o_dep = (o_k + (size_t)n * sizeof(coeb_keypoint) + 255) & ~(size_t)255;
    const size_t o_out = (o_dep + (size_t)W * H * 4 + 255) & ~(size_t)255;
    if ((rc = pinned(c, o_out + (size_t)n * 8))) return rc;
    memcpy(c->pin + o_n, &n, 4);
    memcpy(c->pin + o_k, kps, (size_t)n * sizeof(coeb_keypoint));
    float* hdep = reinterpret_cast<float*>(c->pin + o_dep);
    if (dstride == (size_t)W) memcpy(hdep, depth, (size_t)W * H * 4);
    else
        for (int y = 0; y < H; y++) memcpy(hdep + (size_t)y * W, depth + (size_t)y * dstride, (size_t)W * 4);
    PrepBufs pb;
    memset(&pb, 0, sizeof(pb));
    pb.kps = c->pin_dev + o_k;
    pb.n = reinterpret_cast<const int32_t*>(c->pin_dev + o_n);
    pb.stride = n; pb.depth = reinterpret_cast<const float*>(c->pin_dev + o_dep); pb.W = W; pb.H = H;
    pb.bf = bf; pb.fx = 1; pb.fy = 1;
    pb.ur = reinterpret_cast<float*>(c->pin_dev + o_out);
    pb.dep = reinterpret_cast<float*>(c->pin_dev + o_out) + n;
    if (launch_prep(pb, 1, s, &c->hook)) return hip_err(c, hipGetLastError(), "launch_prep");
    HIP_TRY(c, hipStreamSynchronize(s));
    memcpy(ur_out, c->pin + o_out, (size_t)n * 4);
    memcpy(dep_out, c->pin + o_out + (size_t)n * 4, (size_t)n * 4);
    return COEB_OK;
}

int coeb_descriptor_distance(const uint8_t* a, const uint8_t* b)
{
    // ORBmatcher::DescriptorDistance (ORBmatcher.cc:1648-1664): 8 x 32-bit XOR + popcount.
    // Kept on the CPU: it is also called one pair at a time from MapPoint/Frame code.
    int d = 0;
    for (int i = 0; i < 8; i++) {
        uint32_t x, y;
        memcpy(&x, a + 4 * i, 4);
        memcpy(&y, b + 4 * i, 4);
        d += __builtin_popcount(x ^ y);
    }
    return d;
}

int coeb_profile_enable(coeb_ctx* c, int enable)
{
    if (!c) return COEB_EINVAL;
    c->prof.enabled = enable != 0;
    return COEB_OK;
}

int coeb_profile_reset(coeb_ctx* c)
{
    if (!c) return COEB_EINVAL;
    (void)hipSetDevice(c->device);
    c->prof.drain();
    std::fill(c->prof.ms.begin(), c->prof.ms.end(), 0.0);
    std::fill(c->prof.launches.begin(), c->prof.launches.end(), 0);
    return COEB_OK;
}

int coeb_profile_read(coeb_ctx* c, char* names, int cap, double* total_ms, int64_t* launches, int max_k, int* nk)
{
    if (!c) return COEB_EINVAL;
    (void)hipSetDevice(c->device);
    c->prof.drain();
    std::string s;
    const int k = std::min<int>(max_k, (int)c->prof.names.size());
    for (int i = 0; i < k; i++) {
        if (i) s += ",";
        s += c->prof.names[i];
        if (total_ms) total_ms[i] = c->prof.ms[i];
        if (launches) launches[i] = c->prof.launches[i];
    }
    if (names && cap > 0) {
        strncpy(names, s.c_str(), cap - 1);
        names[cap - 1] = 0;
    }
    if (nk) *nk = k;
    return COEB_OK;
}

int coeb_device_alloc(coeb_ctx* c, size_t bytes, void** dptr)
{
    if (!c || !dptr) return COEB_EINVAL;
    (void)hipSetDevice(c->device);
    hipError_t e = hipMalloc(dptr, std::max<size_t>(bytes, 1));
    if (e != hipSuccess) return set_err(c, COEB_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    return COEB_OK;
}

int coeb_device_free(coeb_ctx* c, void* dptr)
{
    if (!c) return COEB_EINVAL;
    (void)hipSetDevice(c->device);
    HIP_TRY(c, hipStreamSynchronize(main_stream(c)));
    if (dptr) HIP_TRY(c, hipFree(dptr));
    return COEB_OK;
}

int coeb_memcpy_h2d(coeb_ctx* c, void* dst, const void* src, size_t bytes)
{
    if (!c || (bytes && (!dst || !src))) return COEB_EINVAL;
    (void)hipSetDevice(c->device);
    HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, main_stream(c)));
    HIP_TRY(c, hipStreamSynchronize(main_stream(c)));
    return COEB_OK;
}

int coeb_memcpy_d2h(coeb_ctx* c, void* dst, const void* src, size_t bytes)
{
    if (!c || (bytes && (!dst || !src))) return COEB_EINVAL;
    (void)hipSetDevice(c->device);
    join_pose(c);
    HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, main_stream(c)));
    HIP_TRY(c, hipStreamSynchronize(main_stream(c)));
    return COEB_OK;
}

int coeb_host_alloc(size_t bytes, void** ptr)
{
    if (!ptr) return COEB_EINVAL;
    hipError_t e = hipHostMalloc(ptr, std::max<size_t>(bytes, 1), hipHostMallocDefault);
    if (e != hipSuccess) return set_err(nullptr, COEB_ENOMEM, std::string("hipHostMalloc: ") + hipGetErrorString(e));
    return COEB_OK;
}

int coeb_host_free(void* ptr)
{
    if (ptr && hipHostFree(ptr) != hipSuccess) return set_err(nullptr, COEB_EDEVICE, "hipHostFree failed");
    return COEB_OK;
}

int coeb_memcpy_h2d_async(coeb_ctx* c, void* dst, const void* src, size_t bytes)
{
    if (!c || (bytes && (!dst || !src))) return COEB_EINVAL;
    (void)hipSetDevice(c->device);
    HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, main_stream(c)));
    return COEB_OK;
}

int coeb_memcpy_d2h_async(coeb_ctx* c, void* dst, const void* src, size_t bytes)
{
    if (!c || (bytes && (!dst || !src))) return COEB_EINVAL;
    (void)hipSetDevice(c->device);
    join_pose(c);
    HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, main_stream(c)));
    return COEB_OK;
}

// ---- copy queues: a stream of their own beside a context's stream (coeb_front.h) ----
// Each ordering call records a fresh event of a small ring: re-recording one event object while
// another stream still waits on its earlier record measured as a false dependency.
constexpr int kCopyqEvents = 16;
struct coeb_copyq {
    int device = 0;
    hipStream_t s = nullptr;
    hipEvent_t ev[kCopyqEvents] = {};
    int next = 0;
    hipEvent_t take() { hipEvent_t e = ev[next]; next = (next + 1) % kCopyqEvents; return e; }
};

coeb_copyq* coeb_copyq_create(coeb_ctx* c)
{
    if (!c) return nullptr;
    (void)hipSetDevice(c->device);
    coeb_copyq* q = new coeb_copyq;
    q->device = c->device;
    bool ok = hipStreamCreateWithFlags(&q->s, hipStreamNonBlocking) == hipSuccess;
    for (int i = 0; ok && i < kCopyqEvents; i++) ok = hipEventCreateWithFlags(&q->ev[i], hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        set_err(c, COEB_EDEVICE, "coeb_copyq_create: stream / event creation failed");
        for (hipEvent_t e : q->ev)
            if (e) (void)hipEventDestroy(e);
        if (q->s) (void)hipStreamDestroy(q->s);
        delete q;
        return nullptr;
    }
    return q;
}

int coeb_copyq_destroy(coeb_copyq* q)
{
    if (!q) return COEB_OK;
    (void)hipSetDevice(q->device);
    (void)hipStreamSynchronize(q->s);
    for (hipEvent_t e : q->ev) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(q->s);
    delete q;
    return COEB_OK;
}

int coeb_copyq_h2d(coeb_copyq* q, void* dst, const void* src, size_t bytes)
{
    if (!q || (bytes && (!dst || !src))) return COEB_EINVAL;
    (void)hipSetDevice(q->device);
    if (hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, q->s) != hipSuccess)
        return set_err(nullptr, COEB_EDEVICE, "coeb_copyq_h2d: hipMemcpyAsync failed");
    return COEB_OK;
}

int coeb_copyq_d2h(coeb_copyq* q, void* dst, const void* src, size_t bytes)
{
    if (!q || (bytes && (!dst || !src))) return COEB_EINVAL;
    (void)hipSetDevice(q->device);
    if (hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, q->s) != hipSuccess)
        return set_err(nullptr, COEB_EDEVICE, "coeb_copyq_d2h: hipMemcpyAsync failed");
    return COEB_OK;
}

int coeb_copyq_after_ctx(coeb_copyq* q, coeb_ctx* c)
{
    if (!q || !c || q->device != c->device) return COEB_EINVAL;
    (void)hipSetDevice(c->device);
    hipStream_t s = main_stream(c);
    join_pose(c);
    hipEvent_t e = q->take();
    HIP_TRY(c, hipEventRecord(e, s));
    HIP_TRY(c, hipStreamWaitEvent(q->s, e, 0));
    return COEB_OK;
}

int coeb_ctx_after_copyq(coeb_ctx* c, coeb_copyq* q)
{
    if (!q || !c || q->device != c->device) return COEB_EINVAL;
    (void)hipSetDevice(c->device);
    hipEvent_t e = q->take();
    HIP_TRY(c, hipEventRecord(e, q->s));
    HIP_TRY(c, hipStreamWaitEvent(main_stream(c), e, 0));
    return COEB_OK;
}

int coeb_copyq_synchronize(coeb_copyq* q)
{
    if (!q) return COEB_EINVAL;
    (void)hipSetDevice(q->device);
    if (hipStreamSynchronize(q->s) != hipSuccess) return set_err(nullptr, COEB_EDEVICE, "coeb_copyq_synchronize failed");
    return COEB_OK;
}

// ---- markers (coeb_front.h): one HIP event, recorded on a context's or queue's stream ----
struct coeb_marker {
    int device = 0;
    hipEvent_t ev = nullptr;
};

coeb_marker* coeb_marker_create(coeb_ctx* c)
{
    if (!c) return nullptr;
    (void)hipSetDevice(c->device);
    coeb_marker* m = new coeb_marker;
    m->device = c->device;
    if (hipEventCreateWithFlags(&m->ev, hipEventDisableTiming) != hipSuccess) {
        set_err(c, COEB_EDEVICE, "coeb_marker_create: event creation failed");
        delete m;
        return nullptr;
    }
    return m;
}

int coeb_marker_destroy(coeb_marker* m)
{
    if (!m) return COEB_OK;
    (void)hipSetDevice(m->device);
    (void)hipEventSynchronize(m->ev);
    (void)hipEventDestroy(m->ev);
    delete m;
    return COEB_OK;
}

int coeb_marker_record_ctx(coeb_marker* m, coeb_ctx* c)
{
    if (!m || !c || m->device != c->device) return COEB_EINVAL;
    (void)hipSetDevice(c->device);
    hipStream_t s = main_stream(c);          // joins pending side-stream work first
    join_pose(c);
    HIP_TRY(c, hipEventRecord(m->ev, s));
    return COEB_OK;
}

int coeb_marker_record_copyq(coeb_marker* m, coeb_copyq* q)
{
    if (!m || !q || m->device != q->device) return COEB_EINVAL;
    (void)hipSetDevice(q->device);
    if (hipEventRecord(m->ev, q->s) != hipSuccess) return set_err(nullptr, COEB_EDEVICE, "coeb_marker_record_copyq failed");
    return COEB_OK;
}

int coeb_ctx_wait_marker(coeb_ctx* c, coeb_marker* m)
{
    if (!m || !c || m->device != c->device) return COEB_EINVAL;
    (void)hipSetDevice(c->device);
    HIP_TRY(c, hipStreamWaitEvent(main_stream(c), m->ev, 0));
    return COEB_OK;
}

int coeb_copyq_wait_marker(coeb_copyq* q, coeb_marker* m)
{
    if (!m || !q || m->device != q->device) return COEB_EINVAL;
    (void)hipSetDevice(q->device);
    if (hipStreamWaitEvent(q->s, m->ev, 0) != hipSuccess) return set_err(nullptr, COEB_EDEVICE, "coeb_copyq_wait_marker failed");
    return COEB_OK;
}

int coeb_marker_synchronize(coeb_marker* m)
{
    if (!m) return COEB_EINVAL;
    (void)hipSetDevice(m->device);
    if (hipEventSynchronize(m->ev) != hipSuccess) return set_err(nullptr, COEB_EDEVICE, "coeb_marker_synchronize failed");
    return COEB_OK;
}

/* Debug readback of intermediate buffers of frame f of the last batch (test support):
 * what = "pyr" | "blur" | "cand_n" | "lvl_n" | "lvl_kp" | "dyn" | "u_right" | "kp_depth"; copies
 * min(bytes, size).
 * Of the context's last moving-object batch (coeb_frame_batch_device with F >= 2; both refuse with
 * COEB_EINVAL when there is none, or a single-pair flow call has rewritten the flow scratch since):
 *   "flow_counts": [pairs][2] int32 {Harris candidate keys, corners}, f ignored;
 *   "flow_pair":   pair f (frames f, f + 1; COEB_EINVAL outside 0 .. pairs - 1) as one fixed record
 *                  (FlowPairRecord): int32 npts, int32 nf, double F[9], float pts[1024][2] (sub-pixel
 *                  corners), float nxt[1024][2] (LK next points), uint8 status[1024] (LK),
 *                  uint8 state[1024] (after the SAD / edge test); entries past npts, and F when
 *                  findFundamentalMat returned none, are whatever the scratch held.
 * Both synchronise the context stream. */
int coeb_debug_read(coeb_ctx* c, const char* what, int f, void* host, size_t bytes, size_t* size_out)
{
    if (c) join_pose(c);
    if (c && what && std::string(what) == "fast_timing") {
        // [8] k_fast phase clocks (COEB_FAST_CLOCK builds)
        unsigned long long t[8];
        if (size_out) *size_out = sizeof(t);
        if (!host) return 0;                         // size query: the read below also clears
        if (fast_timing_read(t)) return COEB_EDEVICE;
        memcpy(host, t, std::min(bytes, sizeof(t)));
        return 0;
    }
    if (c && what && std::string(what) == "flow_counts") {     // [pairs][2] {Harris keys, corners}
        static thread_local int t[2 * 8192];
        int np = 0;
        int rc = flow_counts(c, t, 2 * 8192, &np);
        if (rc) return rc;
        const size_t n = (size_t)std::min(np, 8192) * 8;
        if (size_out) *size_out = n;
        if (host) memcpy(host, t, std::min(bytes, n));
        return COEB_OK;
    }
    if (c && what && std::string(what) == "flow_pair") {       // FlowPairRecord of pair f (coeb_ctx.hpp)
        static thread_local FlowPairRecord rec;
        int rc = flow_pair(c, f, &rec);
        if (rc) return rc;
        if (size_out) *size_out = sizeof(rec);
        if (host) memcpy(host, &rec, std::min(bytes, sizeof(rec)));
        return COEB_OK;
    }
    if (c && what && std::string(what) == "oct_timing") {      // [4096][6] k_octree clocks (COEB_OCT_CLOCK)
        static long long t[4096 * 6];
        if (size_out) *size_out = sizeof(t);
        if (!host) return 0;
        HIP_TRY(c, hipStreamSynchronize(main_stream(c)));
        if (oct_timing_read(t)) return COEB_EDEVICE;
        memcpy(host, t, std::min(bytes, sizeof(t)));
        return 0;
    }
    if (c && what && (std::string(what) == "pose_timing" || std::string(what) == "match_timing")) {
        // [F][8] k_pose phase clocks (COEB_POSE_CLOCK builds) / [F][16] k_match phase clocks (COEB_MATCH_CLOCK builds)
        const DevArr<long long>& t = what[0] == 'p' ? c->tim.p_timing : c->tim.m_timing;
        if (!t.p) return COEB_EINVAL;
        if (size_out) *size_out = t.bytes;
        if (host && bytes) {
            HIP_TRY(c, hipStreamSynchronize(main_stream(c)));
            HIP_TRY(c, hipMemcpy(host, t.p, std::min(bytes, t.bytes), hipMemcpyDeviceToHost));
        }
        return COEB_OK;
    }
    if (c && what && (std::string(what) == "search_path" || std::string(what) == "localmap_path")) {
        // {path, iterations} of the last coeb_match_localmap / coeb_match_keyframe / coeb_search_local_points /
        // coeb_track_local_map
        if (!c->sf.l_path.p) return COEB_EINVAL;
        if (size_out) *size_out = 8;
        if (host && bytes) {
            HIP_TRY(c, hipStreamSynchronize(main_stream(c)));
            HIP_TRY(c, hipMemcpy(host, c->sf.l_path.p, std::min(bytes, (size_t)8), hipMemcpyDeviceToHost));
        }
        return COEB_OK;
    }
    if (!c || !what || !c->has_plan || f < 0 || f >= c->batch_frames) return COEB_EINVAL;
    (void)hipSetDevice(c->device);
    const Plan& P = c->plan;
    const uint8_t* src = nullptr;
    size_t n = 0;
    std::string w(what);
    if (w == "pyr") { src = c->ex.pyr.p + (size_t)f * P.pyr_stride; n = P.pyr_stride; }
    else if (w == "blur") {
        // the blurred levels row-major at their pitch, each 256-B aligned (the device copy is tiled,
        // blur_tile_off)
        std::vector<uint8_t> raw(P.blur_stride);
        HIP_TRY(c, hipStreamSynchronize(main_stream(c)));
        HIP_TRY(c, hipMemcpy(raw.data(), c->ex.blur.p + (size_t)f * P.blur_stride, raw.size(),
                             hipMemcpyDeviceToHost));
        std::vector<uint8_t> rm;
        size_t off = 0;
        for (int l = 0; l < P.L; l++) {
            const LevelGeom& g = P.lv[l];
            rm.resize(off + (size_t)g.bpitch * g.h);
            for (int y = 0; y < g.h; y++)
                for (int x = 0; x < g.bpitch; x++)
                    rm[off + (size_t)y * g.bpitch + x] = raw[g.blur_off + blur_tile_off(x, y, g.bpitch)];
            off = ((off + (size_t)g.bpitch * g.h) + 255) & ~(size_t)255;
        }
        rm.resize(off);
        if (size_out) *size_out = rm.size();
        if (host && bytes) memcpy(host, rm.data(), std::min(bytes, rm.size()));
        return COEB_OK;
    }
    else if (w == "cand_n") { src = (const uint8_t*)c->ex.cand_n.p + (size_t)f * P.ncells * 4; n = (size_t)P.ncells * 4; }
    else if (w == "lvl_n") { src = (const uint8_t*)c->ex.lvl_n.p + (size_t)f * P.L * 4; n = (size_t)P.L * 4; }
    else if (w == "lvl_kp") { src = (const uint8_t*)c->ex.lvl_kp.p + (size_t)f * P.lvl_stride * 4; n = (size_t)P.lvl_stride * 4; }
    else if (w == "dyn") { src = (const uint8_t*)c->ex.dyn.p + (size_t)f * sizeof(DynMask); n = sizeof(DynMask); }
    else if (w == "u_right" || w == "kp_depth") {
        // k_prep's mvuRight / mvDepth of frame f's kcap keypoint slots (the last batch matcher's)
        const DevArr<float>& a = w == "u_right" ? c->bm.b_ur : c->bm.b_dep;
        if (!a.p || a.bytes < (size_t)c->batch_frames * P.kcap * 4) return COEB_EINVAL;
        src = (const uint8_t*)(a.p + (size_t)f * P.kcap); n = (size_t)P.kcap * 4;
    }
    else if (w == "plan") { if (size_out) *size_out = sizeof(Plan); if (host) memcpy(host, &P, std::min(bytes, sizeof(Plan))); return COEB_OK; }
    else return COEB_EINVAL;
    if (size_out) *size_out = n;
    if (host && bytes) {
        HIP_TRY(c, hipStreamSynchronize(main_stream(c)));
        HIP_TRY(c, hipMemcpy(host, src, std::min(bytes, n), hipMemcpyDeviceToHost));
    }
    return COEB_OK;
}

int coeb_synchronize(coeb_ctx* c)
{
    if (!c) return COEB_EINVAL;
    (void)hipSetDevice(c->device);
    join_pose(c);
    HIP_TRY(c, hipStreamSynchronize(main_stream(c)));
    return check_err_word(c);
}

}  // extern "C"
