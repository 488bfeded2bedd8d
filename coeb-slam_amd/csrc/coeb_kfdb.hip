// coeb_kfdb.hip -- the keyframe database of Tracking::Relocalization on the device:
//   KeyFrameDatabase::add / erase / clear                src/KeyFrameDatabase.cc:40-73
//   DetectRelocalizationCandidates up to lScoreAndMatch  src/KeyFrameDatabase.cc:199-253
//                                                        (k_kfdb_common, k_kfdb_score)
//   SearchByBoW against every candidate                  src/Tracking.cc:1449-1470 (k_match_bow_db)
//   SearchForTriangulation against every neighbour       src/ORBmatcher.cc:657-824, 140-157 (k_tri_match,
//                                                        k_tri_rot)
//   the loop body of CreateNewMapPoints behind it        src/LocalMapping.cc:285-433, src/KeyFrame.cc:615-631
//                                                        (k_tri_points)
//   the search of ORBmatcher::Fuse for many (keyframe,   src/ORBmatcher.cc:826-951, src/KeyFrame.cc:569-608
//   point list) pairs                                    (k_fuse_grid, k_fuse)
// What a keyframe contributes never changes after KeyFrame::ComputeBoW, so it is uploaded once
// (descriptors, angles, BowVector) and its feature-vector CSR is built once.  There is no inverted
// file: mnRelocWords of a keyframe is |words(F) & words(KF)|, counted per keyframe.  The scoring
// restates DBoW2's L1Scoring; parity against DBoW2 itself is UNPINNED.
#include <hip/hip_runtime.h>

#include <array>
#include <climits>
#include <cstring>
#include <vector>

#include "coeb_bow_dev.hpp"
#include "coeb_kfdb_host.hpp"
#include "coeb_track_dev.hpp"

// One slot of the slab, by byte offset (mf = max_features): value[mf] f64, word[mf] i32,
// angle[mf] f32, descriptor[mf][32], the CSR (csr_ints(mf) ints, laid out for the keyframe's own n).
struct KfdbView {
    uint8_t* slab;
    size_t stride;
    int* meta;              // [slot][4]: n, nw, 0, 0 (an empty slot: all 0)
    int mf;
    __host__ __device__ double* value(int slot) const { return reinterpret_cast<double*>(slab + slot * stride); }
    __host__ __device__ int* word(int slot) const { return reinterpret_cast<int*>(slab + slot * stride + (size_t)mf * 8); }
    __host__ __device__ float* angle(int slot) const { return reinterpret_cast<float*>(slab + slot * stride + (size_t)mf * 12); }
    __host__ __device__ uint8_t* desc(int slot) const { return slab + slot * stride + (size_t)mf * 16; }
    __host__ __device__ int* csr(int slot) const { return reinterpret_cast<int*>(slab + slot * stride + (size_t)mf * 48); }
};

// One device array of the database: `stride` bytes per slot, `cap` slots.  stride 0: not in use, never
// allocated; p is null before the first allocation and after release_device.
struct KfdbSlab {
    uint8_t* p = nullptr;
    size_t stride = 0;
};
// The database's device memory: the keyframe slots (KfdbView), meta[slot][4], and the two arrays the
// first call that needs them adds (lazy_slab) -- KfdbGeo[mf] per slot (coeb_kfdb_set_geometry), the
// keyframe's 64 x 48 feature grid as a CSR, fuse_grid_ints(mf) ints per slot (coeb_kfdb_fuse_search), and
// KfdbStereo[mf] per slot (coeb_kfdb_set_stereo).
enum { kSlab, kMeta, kGeo, kGrid, kStereo, kNumSlabs };
using KfdbSlabs = std::array<KfdbSlab, kNumSlabs>;

struct coeb_kfdb {
    coeb_ctx* c = nullptr;          // null once the context is gone
    KfdbSlabs sl;
    int mf = 0;                     // max_features
    int cap = 0;                    // allocated slots
    int nslots = 0;                 // one past the highest slot handed out
    int nkf = 0;
    int64_t next_seq = 0;
    std::vector<uint8_t> used;
    std::vector<int> n, nd;         // features and feature-vector nodes per slot
    std::vector<int64_t> seq;       // insertion sequence number per slot
    std::vector<uint8_t> has_geo;   // the slot's keyframe has its geometry
    std::vector<KfdbGridRec> grid_rec;      // the bounds each slot's grid was built with
    std::vector<uint8_t> has_st;    // the slot's keyframe has its stereo data
    std::vector<uint8_t> st_conflict;       // ... and a feature with u_right >= 0 and depth <= 0
    std::vector<std::vector<uint8_t> > is_stereo, depth_pos;    // u_right >= 0 / depth > 0 per feature, as uploaded
    // has_geo / has_st of a slot go to 0, with what hangs on them
    void drop(int slot)
    {
        has_geo[slot] = has_st[slot] = st_conflict[slot] = 0;
        grid_rec[slot].built = 0;
        is_stereo[slot].clear();
        depth_pos[slot].clear();
    }
    void note_conflict(int slot)
    {
        st_conflict[slot] = has_geo[slot] && has_st[slot] &&
                            kfdb_stereo_conflict(is_stereo[slot].data(), depth_pos[slot].data(), n[slot]);
    }
    KfdbView view() const { return KfdbView{sl[kSlab].p, sl[kSlab].stride, reinterpret_cast<int*>(sl[kMeta].p), mf}; }
};

namespace {

constexpr int kDbThreads = 256;
constexpr int kDbWaves = kDbThreads / 64;
constexpr int kQMax = 4096;             // > kBowMax query words
constexpr int kMaxCand = 256;

// ============================= k_kfdb_store =============================
// The staged keyframe into its slot: four runs of 4-byte words and the slot's meta entry.
struct StoreSeg { const uint32_t* src; uint32_t* dst; int n; };
struct StoreArgs { StoreSeg seg[4]; int* meta; int n, nw; };

__global__ __launch_bounds__(kDbThreads) void k_kfdb_store(StoreArgs a)
{
    const int t = blockIdx.x * kDbThreads + threadIdx.x, T = gridDim.x * kDbThreads;
#pragma unroll
    for (int k = 0; k < 4; k++)
        for (int i = t; i < a.seg[k].n; i += T) a.seg[k].dst[i] = a.seg[k].src[i];
    if (t == 0) { a.meta[0] = a.n; a.meta[1] = a.nw; a.meta[2] = 0; a.meta[3] = 0; }
}

// position of w in the ascending s[0 .. n), or -1
__device__ __forceinline__ int find_word(const int* s, int n, int w)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s[mid] < w) lo = mid + 1;
        else hi = mid;
    }
    return (lo < n && s[lo] == w) ? lo : -1;
}

// ============================= k_kfdb_common =============================
// One wave per slot, the query's word ids in LDS.  Lane l takes the keyframe's words l, l + 64, ..
// and searches each in the query; the wave reduces the count (mnRelocWords) and the smallest
// common word (where the inverted file meets the keyframe first); hdr[0] = the maximum count.
__global__ __launch_bounds__(kDbThreads) void k_kfdb_common(KfdbView v, int nslots, const int* __restrict__ qword, int nw,
                                                            int* hdr, int* common, int* first)
{
    __shared__ int s_q[kQMax];
    for (int i = threadIdx.x; i < nw; i += kDbThreads) s_q[i] = qword[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, slot = blockIdx.x * kDbWaves + (threadIdx.x >> 6);
    if (slot >= nslots) return;                    // wave-uniform
    const int knw = v.meta[slot * 4 + 1];
    const int* kw = v.word(slot);
    int cnt = 0, fw = INT_MAX;
    for (int i = lane; i < knw; i += 64) {
        const int w = kw[i];
        if (find_word(s_q, nw, w) >= 0) { cnt++; fw = min(fw, w); }
    }
#pragma unroll
    for (int x = 1; x < 64; x <<= 1) {
        cnt += __shfl_xor(cnt, x);
        fw = min(fw, __shfl_xor(fw, x));
    }
    if (lane == 0) {
        common[slot] = cnt;
        first[slot] = fw;
        if (cnt > 0) atomicMax(&hdr[0], cnt);
    }
}

// ============================= k_kfdb_score =============================
// L1Scoring::score(F, KF) of the slots with common > minCommonWords, one wave per slot.
// minCommonWords comes from hdr[0] with the reference's float multiply and truncation, here on
// the device (no host round trip after k_kfdb_common); hdr[1] keeps it for the host.
// The score is a double sum over the common words in ascending word order, and the float result
// must be the one a sequential sum gives: per 64 keyframe words the lanes evaluate their terms
// fabs(vi - wi) - fabs(vi) - fabs(wi) in parallel and compact them, in word order, into LDS by
// ballot and prefix count; lane 0 then adds them one after the other.  That chain is serial on
// purpose -- a tree reduction rounds differently.  A term has no multiply, so there is nothing
// for floating-point contraction to fuse.
__global__ __launch_bounds__(kDbThreads) void k_kfdb_score(KfdbView v, int nslots, const int* __restrict__ qword,
                                                           const double* __restrict__ qvalue, int nw, int* hdr,
                                                           const int* __restrict__ common, float* score)
{
    __shared__ int s_q[kQMax];
    __shared__ double s_v[kQMax];
    __shared__ double s_t[kDbWaves][64];
    const int max_common = hdr[0];
    const int min_common = (int)((float)max_common * 0.8f);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, slot = blockIdx.x * kDbWaves + wv;
    const bool scored = slot < nslots && common[slot] > min_common;
    if (slot < nslots && !scored && lane == 0) score[slot] = -1.0f;
    if (!__syncthreads_or(scored)) {               // most workgroups end here
        if (blockIdx.x == 0 && threadIdx.x == 0) hdr[1] = min_common;
        return;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) hdr[1] = min_common;
    for (int i = threadIdx.x; i < nw; i += kDbThreads) { s_q[i] = qword[i]; s_v[i] = qvalue[i]; }
    __syncthreads();
    if (!scored) return;                           // wave-uniform
    const int knw = v.meta[slot * 4 + 1];
    const int* kw = v.word(slot);
    const double* kv = v.value(slot);
    double s = 0.0;                                // lane 0's
    for (int base = 0; base < knw; base += 64) {
        const int i = base + lane;
        bool hit = false;
        double term = 0.0;
        if (i < knw) {
            const int pos = find_word(s_q, nw, kw[i]);
            if (pos >= 0) {
                const double vi = s_v[pos], wi = kv[i];
                term = fabs(vi - wi) - fabs(vi) - fabs(wi);
                hit = true;
            }
        }
        const uint64_t m = __ballot(hit);
        if (hit) s_t[wv][__popcll(m & (((uint64_t)1 << lane) - 1))] = term;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (lane == 0) {
            const int cnt = __popcll(m);
            for (int k = 0; k < cnt; k++) s += s_t[wv][k];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();           // the next 64 words overwrite s_t
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if (lane == 0) score[slot] = (float)(-s / 2.0);
}

// ============================ k_match_bow_db ============================
// k_match_bow over (keyframe node, candidate): the keyframe side comes from the candidate's slot
// (its CSR lists every feature with a node; valid is tested in the walk), the frame side is one
// CSR for all candidates; matches, rotation bins and histograms are per candidate.
struct DbMatch {
    KfdbView v;
    const int* cand;            // [ncand][2]: slot, byte offset of the candidate's valid mask in stage
    const uint8_t* stage;
    BowSide cur;
    float nnratio;
    int check_ori;
    int cs;                     // max(cur.n, 1): the row stride of match and bin
    int* match; int* bin; int* hist; int* nm;
};

__global__ __launch_bounds__(kBowThreads) void k_match_bow_db(DbMatch a)
{
    __shared__ uint32_t s_desc[kBowWaves][8][kTile];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, y = blockIdx.y;
    const int slot = a.cand[2 * y];
    const BowSide kf{a.v.desc(slot), a.v.angle(slot), a.v.csr(slot), a.v.meta[slot * 4]};
    bow_match_node<true>(kf, a.cur, a.stage + a.cand[2 * y + 1], blockIdx.x * kBowWaves + wv, a.nnratio, a.check_ori,
                         a.match + (size_t)y * a.cs, a.bin + (size_t)y * a.cs, a.hist + y * 32, s_desc[wv], lane);
}

// the three-maxima pass and the match count of every candidate, one workgroup each
__global__ __launch_bounds__(kCsrThreads) void k_bow_rot_db(DbMatch a)
{
    __shared__ int s_ind[3], s_cnt;
    const int y = blockIdx.x;
    bow_rot_filter(a.match + (size_t)y * a.cs, a.bin + (size_t)y * a.cs, a.hist + y * 32, a.cur.n, a.check_ori, a.nm + y,
                   s_ind, &s_cnt);
}

// ============================== k_tri_match ==============================
// ORBmatcher::SearchForTriangulation (:686-776) over (node of keyframe 1, neighbour).  Nothing is
// claimed (:762 is commented out), so a feature idx1 is decided alone: its match is the accepted
// candidate of its node's list in keyframe 2 with the smallest distance, the last in list order
// among equals (dist > bestDist skips, so an equal later one replaces).  bestDist only moves on
// acceptance: a nearer candidate that fails a geometric test shadows nothing.
// A workgroup takes one node; its waves take the node's keyframe-1 features in turn and the lanes
// of a wave the list positions p, p + 64, .. of keyframe 2.  What depends on the candidate alone
// (descriptor, point, the map-point / stereo skip, the epipole test, the chi-square bound) is
// loaded once per lane for the first trip and kept in registers across the wave's features;
// further trips reload theirs.  The winner is one min over (dist << 16 | 0xFFFF - p).  No LDS.
// The float forms are those of the reference binary: a, b = fma(x1, F0k, y1 * F1k)
// + F2k; c = fma(y1, F12, x1 * F02) + F22; den = fma(a, a, b * b); num = fma(b, y2, a * x2) + c;
// the epipole distance fma(dx, dx, dy * dy).  The bound is the double product 3.84 * sigma2.
constexpr int kTriThreads = 256;
constexpr int kTriWaves = kTriThreads / 64;
static_assert(kBowMax <= 0xFFFF, "a list position fits the key's low half");

struct TriArgs {
    KfdbView v;
    const uint8_t* geo;         // the geometry slab
    size_t geo_stride;
    int slot1;
    const uint8_t* has1;        // [n1]
    const int* tab;             // [nnb][2]: slot2, offset of the neighbour's has_mp2 in masks
    const uint8_t* masks;
    const float* F;             // [nnb][9]
    const float* epi;           // [nnb][2]
    const float* scale;         // [COEB_MAXL] mvScaleFactors
    const float* sigma2;        // [COEB_MAXL] mvLevelSigma2
    int only_stereo, check_ori;
    int cs;                     // max(n1, 1): the row stride of match and bin
    int* match; int* bin; int* hist; int* nm;
};

struct TriCand {
    uint32_t d[8];
    float x, y;
    double bound;               // 3.84 * mvLevelSigma2[octave]
    bool ok;                    // in the list, without a MapPoint, stereo under only_stereo
    bool stereo;
    bool near_epipole;          // distex^2 + distey^2 < 100 * mvScaleFactors[octave]
};

__device__ __forceinline__ TriCand tri_cand(const TriArgs& a, const uint8_t* desc2, const KfdbGeo* geo2, const uint8_t* has2,
                                            const int* list2, int p, int len, float ex, float ey)
{
    TriCand c;
#pragma unroll
    for (int k = 0; k < 8; k++) c.d[k] = 0;
    c.x = c.y = 0.f; c.bound = 0.0; c.ok = c.stereo = c.near_epipole = false;
    if (p >= len) return c;
    const int i2 = list2[p];
    const KfdbGeo g = geo2[i2];
    c.stereo = g.u_right >= 0;
    c.ok = !has2[i2] && (!a.only_stereo || c.stereo);
    if (!c.ok) return c;
    const uint4* d = reinterpret_cast<const uint4*>(desc2 + (int64_t)i2 * 32);
    const uint4 d0 = d[0], d1 = d[1];
    c.d[0] = d0.x; c.d[1] = d0.y; c.d[2] = d0.z; c.d[3] = d0.w;
    c.d[4] = d1.x; c.d[5] = d1.y; c.d[6] = d1.z; c.d[7] = d1.w;
    c.x = g.x; c.y = g.y;
    const float distex = ex - g.x, distey = ey - g.y;
    c.near_epipole = fmaf(distex, distex, distey * distey) < 100.0f * a.scale[g.octave];
    c.bound = 3.84 * (double)a.sigma2[g.octave];
    return c;
}

struct TriLine { float a, b, c, den; bool stereo1; };

// the candidate at list position p against one feature of keyframe 1: the smaller of key and its own
__device__ __forceinline__ uint32_t tri_eval(const TriCand& c, int p, const uint32_t* q, const TriLine& l, uint32_t key)
{
    if (!c.ok) return key;
    const uint32_t dist = (uint32_t)hamming32(q, c.d);
    if (dist > (uint32_t)TH_LOW) return key;
    if (!l.stereo1 && !c.stereo && c.near_epipole) return key;
    if (l.den == 0) return key;
    const float num = fmaf(l.b, c.y, l.a * c.x) + l.c;
    const float dsqr = num * num / l.den;
    if (!((double)dsqr < c.bound)) return key;
    return min(key, (dist << 16) | (uint32_t)(0xFFFF - p));
}

__global__ __launch_bounds__(kTriThreads) void k_tri_match(TriArgs a)
{
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int w = blockIdx.x, j = blockIdx.y;
    const int slot2 = a.tab[2 * j];
    const int n1 = a.v.meta[a.slot1 * 4], n2 = a.v.meta[slot2 * 4];
    const int cap1 = max(n1, 1), cap2 = max(n2, 1);
    const int* csr1 = a.v.csr(a.slot1);
    const int* csr2 = a.v.csr(slot2);
    if (w >= csr1[0]) return;                      // workgroup-uniform from here on
    const int* node1 = csr1 + 4;
    const int* off1 = node1 + cap1;
    const int* idx1 = off1 + cap1 + 1;
    const int* node2 = csr2 + 4;
    const int* off2 = node2 + cap2;
    const int* idx2 = off2 + cap2 + 1;
    const int node = node1[w];
    int lo = 0, hi = csr2[0];
    while (lo < hi) {                              // lower bound of node among keyframe 2's nodes
        const int mid = (lo + hi) >> 1;
        if (node2[mid] < node) lo = mid + 1;
        else hi = mid;
    }
    if (lo >= csr2[0] || node2[lo] != node) return;
    const int len = off2[lo + 1] - off2[lo];
    const int* list2 = idx2 + off2[lo];
    const int k0 = off1[w], k1 = off1[w + 1];
    const uint8_t* desc1 = a.v.desc(a.slot1);
    const uint8_t* desc2 = a.v.desc(slot2);
    const KfdbGeo* geo1 = reinterpret_cast<const KfdbGeo*>(a.geo + a.slot1 * a.geo_stride);
    const KfdbGeo* geo2 = reinterpret_cast<const KfdbGeo*>(a.geo + slot2 * a.geo_stride);
    const uint8_t* has2 = a.masks + a.tab[2 * j + 1];
    const float* F = a.F + j * 9;
    const float ex = a.epi[2 * j], ey = a.epi[2 * j + 1];
    const TriCand first = tri_cand(a, desc2, geo2, has2, list2, lane, len, ex, ey);
    for (int kq = k0 + wv; kq < k1; kq += kTriWaves) {
        const int i1 = __builtin_amdgcn_readfirstlane(idx1[kq]);
        if (a.has1[i1]) continue;                  // wave-uniform
        const KfdbGeo g1 = geo1[i1];
        TriLine l;
        l.stereo1 = g1.u_right >= 0;
        if (a.only_stereo && !l.stereo1) continue;
        uint32_t q[8];
        {
            const uint4* d = reinterpret_cast<const uint4*>(desc1 + (int64_t)i1 * 32);
            const uint4 d0 = d[0], d1 = d[1];
            q[0] = d0.x; q[1] = d0.y; q[2] = d0.z; q[3] = d0.w;
            q[4] = d1.x; q[5] = d1.y; q[6] = d1.z; q[7] = d1.w;
        }
        l.a = fmaf(g1.x, F[0], g1.y * F[3]) + F[6];
        l.b = fmaf(g1.x, F[1], g1.y * F[4]) + F[7];
        l.c = fmaf(g1.y, F[5], g1.x * F[2]) + F[8];
        l.den = fmaf(l.a, l.a, l.b * l.b);
        uint32_t key = tri_eval(first, lane, q, l, 0xFFFFFFFFu);
        for (int base = 64; base < len; base += 64)
            key = tri_eval(tri_cand(a, desc2, geo2, has2, list2, base + lane, len, ex, ey), base + lane, q, l, key);
#pragma unroll
        for (int x = 1; x < 64; x <<= 1) key = min(key, (uint32_t)__shfl_xor((int)key, x));
        if (lane == 0 && key != 0xFFFFFFFFu) {
            const int i2 = list2[0xFFFF - (int)(key & 0xFFFFu)];
            a.match[(size_t)j * a.cs + i1] = i2;
            if (a.check_ori) {
                int b = rot_bin(a.v.angle(a.slot1)[i1], a.v.angle(slot2)[i2]);
                if (b < 0 || b >= HISTO_LENGTH) b = HISTO_LENGTH;                // the reference asserts; dropped below
                else atomicAdd(&a.hist[j * 32 + b], 1);
                a.bin[(size_t)j * a.cs + i1] = b;
            }
        }
    }
}

// the three-maxima pass and the match count of every neighbour, one workgroup each
__global__ __launch_bounds__(kCsrThreads) void k_tri_rot(TriArgs a, int n1)
{
    __shared__ int s_ind[3], s_cnt;
    const int y = blockIdx.x;
    bow_rot_filter(a.match + (size_t)y * a.cs, a.bin + (size_t)y * a.cs, a.hist + y * 32, n1, a.check_ori, a.nm + y, s_ind,
                   &s_cnt);
}

// ============================== k_tri_points ==============================
// The loop body of LocalMapping::CreateNewMapPoints (:285-433) for every entry of k_tri_match's rows, one lane
// per (neighbour j = blockIdx.y, feature i of keyframe 1): the views and level tables are the same for a
// whole workgroup, the two feature records come from the geometry and stereo slabs.  Every pair is decided
// alone; first[i] takes the lowest accepted j by an integer atomicMin, which no order of arrival changes.
// No LDS.
// The null vector of the 4x4 system A (:323-332) is the canonical form of DESIGN.md s2.1: a one-sided
// (Hestenes) Jacobi in float32 on A's columns, V accumulated from the identity, the pairs (0,1) (0,2) (0,3)
// (1,2) (1,3) (2,3) in that order, at most kJacobiSweeps sweeps, a pair left alone where |ap.aq| <=
// kJacobiEps * sqrt(|ap|^2 |aq|^2), a lane done after a sweep without a rotation (its own: no lane looks at
// another's); the column of V under the smallest column norm, the last of equals.  A and V stay in
// registers: every index below is a compile-time constant.  It is not cv::SVD's vt.row(3) bit for bit, and
// no test asks that; the sign of the vector cancels in xyz / w.
// Float forms: xn = ((u - cx) * invfx, (v - cy) * invfy, 1) in float; Rwc * xn as cv::Mat's
// small gemm (float products summed left to right), a gemm's addend added in double; Mat::dot and cv::norm
// in double; the rows of A as addWeighted leaves them, fl(xn * T2k) - T0k; x3D / w as a multiply by
// (float)(1.0 / w); z = (float)(dot + tcw[2]); invz = (float)(1.0 / z); u = fma(fx * x, invz, cx), u_r =
// fma(-mbf, invz, u), e2 = fma(ex, ex, ey * ey) then fma(er, er, .), compared in double with the double
// products 5.991 * sigma2 and 7.8 * sigma2; the stereo parallax bound cos(2 atan2(mb / 2, depth)) as
// (d^2 - h^2) / (d^2 + h^2) in double (no libm: it only feeds comparisons).
constexpr int kPtsThreads = 256;
constexpr int kJacobiSweeps = 12;
constexpr float kJacobiEps = 4.76837158203125e-07f;         // 2^-21

struct PtsArgs {
    const uint8_t* geo; size_t geo_stride;
    const uint8_t* st; size_t st_stride;
    int slot1;
    const int* tab;             // [nnb][2]: slot2, (the mask offset)
    const coeb_kf_view* view;   // keyframe 1, then the neighbours
    const float* scale;         // [COEB_MAXL] mvScaleFactors
    const float* sigma2;        // [COEB_MAXL] mvLevelSigma2
    float ratio_factor;
    int n1;
    const int* match;           // [nnb][n1], k_tri_match's
    int8_t* status; float* x3d; int* first;
};

__device__ __forceinline__ float sq4(const float* a)
{
    return __fmaf_rn(a[3], a[3], __fmaf_rn(a[2], a[2], __fmaf_rn(a[1], a[1], a[0] * a[0])));
}

// one pair of columns; true when it was rotated
template <int P, int Q>
__device__ __forceinline__ bool jacobi_pair(float (&a)[4][4], float (&v)[4][4])
{
    const float alpha = sq4(a[P]), beta = sq4(a[Q]);
    const float gamma =
        __fmaf_rn(a[P][3], a[Q][3], __fmaf_rn(a[P][2], a[Q][2], __fmaf_rn(a[P][1], a[Q][1], a[P][0] * a[Q][0])));
    if (fabsf(gamma) <= kJacobiEps * sqrtf(alpha * beta)) return false;
    const float zeta = (beta - alpha) / (2.0f * gamma);
    const float t = copysignf(1.0f, zeta) / (fabsf(zeta) + sqrtf(__fmaf_rn(zeta, zeta, 1.0f)));
    const float c = 1.0f / sqrtf(__fmaf_rn(t, t, 1.0f));
    const float s = c * t;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const float x = a[P][r], y = a[Q][r];
        a[P][r] = __fmaf_rn(c, x, -(s * y));
        a[Q][r] = __fmaf_rn(s, x, c * y);
        const float vx = v[P][r], vy = v[Q][r];
        v[P][r] = __fmaf_rn(c, vx, -(s * vy));
        v[Q][r] = __fmaf_rn(s, vx, c * vy);
    }
    return true;
}

// a[c][r] = A(r, c) on entry; out = the right singular vector of A's smallest singular value
__device__ __forceinline__ void jacobi_null4(float (&a)[4][4], float* out)
{
    float v[4][4];
#pragma unroll
    for (int c = 0; c < 4; c++)
#pragma unroll
        for (int r = 0; r < 4; r++) v[c][r] = c == r ? 1.0f : 0.0f;
    bool active = true;
    for (int sweep = 0; sweep < kJacobiSweeps && active; sweep++) {
        bool rot = jacobi_pair<0, 1>(a, v);
        rot |= jacobi_pair<0, 2>(a, v);
        rot |= jacobi_pair<0, 3>(a, v);
        rot |= jacobi_pair<1, 2>(a, v);
        rot |= jacobi_pair<1, 3>(a, v);
        rot |= jacobi_pair<2, 3>(a, v);
        active = rot;
    }
    float best = sq4(a[0]);
#pragma unroll
    for (int r = 0; r < 4; r++) out[r] = v[0][r];
#pragma unroll
    for (int c = 1; c < 4; c++) {
        const float s = sq4(a[c]);
        if (s <= best) {
            best = s;
#pragma unroll
            for (int r = 0; r < 4; r++) out[r] = v[c][r];
        }
    }
}

// Rwc * x for Rwc = Rcw transposed: cv::Mat's small gemm
__device__ __forceinline__ void rwc_mul(const float* Rcw, const float* x, float* out)
{
#pragma unroll
    for (int k = 0; k < 3; k++) {
        float t = Rcw[0 + k] * x[0] + Rcw[3 + k] * x[1];
        t = t + Rcw[6 + k] * x[2];
        out[k] = t;
    }
}

// Rcw.row(r).dot(x3Dt) + tcw(r), to float
__device__ __forceinline__ float row_dot_add(const coeb_kf_view& V, int r, const float* X)
{
    double d = 0.0;
    d += (double)V.Rcw[3 * r + 0] * (double)X[0];
    d += (double)V.Rcw[3 * r + 1] * (double)X[1];
    d += (double)V.Rcw[3 * r + 2] * (double)X[2];
    return (float)(d + (double)V.tcw[r]);
}

// cos(2 atan2(mb / 2, depth)) = (d^2 - h^2) / (d^2 + h^2)
__device__ __forceinline__ float stereo_parallax_bound(float mb, float depth)
{
    const double h = (double)(mb / 2.0f), d = (double)depth;
    return (float)((d * d - h * h) / (d * d + h * h));
}

// KeyFrame::UnprojectStereo (KeyFrame.cc:615-631); the depth is positive (coeb_kfdb_create_new_map_points refuses otherwise)
__device__ __forceinline__ void unproject_stereo(const coeb_kf_view& V, const KfdbStereo& s, float* X)
{
    const float z = s.depth;
    const float Pc[3] = {(s.kx - V.cx) * z * V.invfx, (s.ky - V.cy) * z * V.invfy, z};
    float t[3];
    rwc_mul(V.Rcw, Pc, t);
#pragma unroll
    for (int k = 0; k < 3; k++) X[k] = (float)((double)t[k] + (double)V.Ow[k]);
}

// the reprojection test of one side (:363-414); mbf is keyframe 1's on both sides (:407)
__device__ __forceinline__ bool reproj_fails(const coeb_kf_view& V, float mbf, const float* X, float z, const KfdbGeo& g,
                                             float sigma2)
{
    const float x = row_dot_add(V, 0, X), y = row_dot_add(V, 1, X);
    const float invz = (float)(1.0 / (double)z);
    const float u = __fmaf_rn(V.fx * x, invz, V.cx), v = __fmaf_rn(V.fy * y, invz, V.cy);
    const float ex = u - g.x, ey = v - g.y;
    float e2 = __fmaf_rn(ex, ex, ey * ey);
    if (!(g.u_right >= 0)) return (double)e2 > 5.991 * (double)sigma2;
    const float er = __fmaf_rn(-mbf, invz, u) - g.u_right;
    e2 = __fmaf_rn(er, er, e2);
    return (double)e2 > 7.8 * (double)sigma2;
}

__global__ __launch_bounds__(kPtsThreads) void k_tri_points(PtsArgs a)
{
    const int i = blockIdx.x * kPtsThreads + threadIdx.x, j = blockIdx.y;
    if (i >= a.n1) return;
    const size_t e = (size_t)j * a.n1 + i;
    const int i2 = a.match[e];
    if (i2 < 0) { a.status[e] = kNpNoPair; return; }
    const int slot2 = a.tab[2 * j];
    const coeb_kf_view& V1 = a.view[0];
    const coeb_kf_view& V2 = a.view[1 + j];
    const KfdbGeo g1 = reinterpret_cast<const KfdbGeo*>(a.geo + a.slot1 * a.geo_stride)[i];
    const KfdbGeo g2 = reinterpret_cast<const KfdbGeo*>(a.geo + slot2 * a.geo_stride)[i2];
    const KfdbStereo s1 = reinterpret_cast<const KfdbStereo*>(a.st + a.slot1 * a.st_stride)[i];
    const KfdbStereo s2 = reinterpret_cast<const KfdbStereo*>(a.st + slot2 * a.st_stride)[i2];
    const bool st1 = g1.u_right >= 0, st2 = g2.u_right >= 0;
    // the parallax between the rays (:300-317)
    const float xn1[3] = {(g1.x - V1.cx) * V1.invfx, (g1.y - V1.cy) * V1.invfy, 1.0f};
    const float xn2[3] = {(g2.x - V2.cx) * V2.invfx, (g2.y - V2.cy) * V2.invfy, 1.0f};
    float ray1[3], ray2[3];
    rwc_mul(V1.Rcw, xn1, ray1);
    rwc_mul(V2.Rcw, xn2, ray2);
    double dot = 0.0;
    dot += (double)ray1[0] * (double)ray2[0];
    dot += (double)ray1[1] * (double)ray2[1];
    dot += (double)ray1[2] * (double)ray2[2];
    const float cos_rays = (float)(dot / (norm3(ray1) * norm3(ray2)));
    float cps1 = cos_rays + 1.0f, cps2 = cps1;
    if (st1) cps1 = stereo_parallax_bound(V1.mb, s1.depth);
    else if (st2) cps2 = stereo_parallax_bound(V2.mb, s2.depth);
    const float cps = cps2 < cps1 ? cps2 : cps1;
    float X[3];
    int src;
    if (cos_rays < cps && cos_rays > 0.0f && (st1 || st2 || (double)cos_rays < 0.9998)) {
        src = COEB_NEWPTS_SRC_TRIANGULATED;
        float A[4][4];                              // A[c][r] = the reference's A(r, c)
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const float t10 = c < 3 ? V1.Rcw[c] : V1.tcw[0], t11 = c < 3 ? V1.Rcw[3 + c] : V1.tcw[1];
            const float t12 = c < 3 ? V1.Rcw[6 + c] : V1.tcw[2];
            const float t20 = c < 3 ? V2.Rcw[c] : V2.tcw[0], t21 = c < 3 ? V2.Rcw[3 + c] : V2.tcw[1];
            const float t22 = c < 3 ? V2.Rcw[6 + c] : V2.tcw[2];
            A[c][0] = xn1[0] * t12 - t10;
            A[c][1] = xn1[1] * t12 - t11;
            A[c][2] = xn2[0] * t22 - t20;
            A[c][3] = xn2[1] * t22 - t21;
        }
        float h[4];
        jacobi_null4(A, h);
        if (h[3] == 0.0f) { a.status[e] = (int8_t)(kNpW0 | (src << 4)); return; }
        const float inv = (float)(1.0 / (double)h[3]);
        X[0] = h[0] * inv; X[1] = h[1] * inv; X[2] = h[2] * inv;
    } else if (st1 && cps1 < cps2) {
        src = COEB_NEWPTS_SRC_STEREO1;
        unproject_stereo(V1, s1, X);
    } else if (st2 && cps2 < cps1) {
        src = COEB_NEWPTS_SRC_STEREO2;
        unproject_stereo(V2, s2, X);
    } else {
        a.status[e] = kNpLowParallax;
        return;
    }
    int code = kNpAccepted;
    const float z1 = row_dot_add(V1, 2, X);
    const float z2 = row_dot_add(V2, 2, X);
    if (z1 <= 0.0f) code = kNpZ1;
    else if (z2 <= 0.0f) code = kNpZ2;
    else if (reproj_fails(V1, V1.mbf, X, z1, g1, a.sigma2[g1.octave])) code = kNpReproj1;
    else if (reproj_fails(V2, V1.mbf, X, z2, g2, a.sigma2[g2.octave])) code = kNpReproj2;
    else {
        const float d1[3] = {X[0] - V1.Ow[0], X[1] - V1.Ow[1], X[2] - V1.Ow[2]};
        const float d2[3] = {X[0] - V2.Ow[0], X[1] - V2.Ow[1], X[2] - V2.Ow[2]};
        const float dist1 = (float)norm3(d1), dist2 = (float)norm3(d2);
        if (dist1 == 0.0f || dist2 == 0.0f) code = kNpZeroDist;
        else {
            const float ratio_dist = dist2 / dist1, ratio_oct = a.scale[g1.octave] / a.scale[g2.octave];
            if (ratio_dist * a.ratio_factor < ratio_oct || ratio_dist > ratio_oct * a.ratio_factor) code = kNpRatio;
        }
    }
    a.status[e] = (int8_t)(code | (src << 4));
    if (code == kNpAccepted) {
        a.x3d[3 * e] = X[0]; a.x3d[3 * e + 1] = X[1]; a.x3d[3 * e + 2] = X[2];
        atomicMin(&a.first[i], j);
    }
}

// ============================== k_fuse_grid ==============================
// Frame::AssignFeaturesToGrid (Frame.cc:396-411; a KeyFrame copies the Frame's grid) of one stored
// keyframe per workgroup, as a CSR in cell order (ix outer, iy inner, index order inside a cell):
// cell[c] = the start of cell c = ix * 48 + iy in sorted[], cell[3072] = the listed features.  A feature
// whose PosInGrid (round) falls outside the grid is listed nowhere.  The counting sort is that of
// stage_grid (coeb_match.hip): counts by LDS atomics, a block scan, a scatter through per-cell cursors
// and an insertion sort of every (short) cell range, since the scatter's order inside a cell is any.
constexpr int kGridThreads = 256;
constexpr int kGridCpt = COEB_GRID_CELLS / kGridThreads;
static_assert(COEB_GRID_CELLS == kGridCpt * kGridThreads, "whole cells per thread");
inline size_t fuse_grid_ints(int mf) { return (size_t)COEB_GRID_CELLS + 1 + (size_t)mf; }

struct FuseGridArgs {
    KfdbView v;
    const uint8_t* geo; size_t geo_stride;
    uint8_t* grid; size_t grid_stride;
    const int* slots;           // [gridDim.x]
    float min_x, min_y, inv_w, inv_h;
};

__global__ __launch_bounds__(kGridThreads) void k_fuse_grid(FuseGridArgs a)
{
    __shared__ int s_start[COEB_GRID_CELLS + 1];
    __shared__ int s_cur[COEB_GRID_CELLS];
    __shared__ int s_sort[kBowMax + 1];
    __shared__ int s_wsum[kGridThreads / 64];
    const int tid = threadIdx.x, slot = a.slots[blockIdx.x];
    const int n = min(a.v.meta[slot * 4], a.v.mf);
    const KfdbGeo* geo = reinterpret_cast<const KfdbGeo*>(a.geo + slot * a.geo_stride);
    int* cell = reinterpret_cast<int*>(a.grid + slot * a.grid_stride);
    int* sorted = cell + COEB_GRID_CELLS + 1;
    const auto cell_of = [&](int i) {
        const KfdbGeo g = geo[i];
        const int px = (int)roundf((g.x - a.min_x) * a.inv_w);          // PosInGrid (Frame.cc:560-571)
        const int py = (int)roundf((g.y - a.min_y) * a.inv_h);
        return (px >= 0 && px < COEB_GRID_COLS && py >= 0 && py < COEB_GRID_ROWS) ? px * COEB_GRID_ROWS + py : -1;
    };
    for (int c = tid; c <= COEB_GRID_CELLS; c += kGridThreads) s_start[c] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += kGridThreads) {
        const int c = cell_of(i);
        if (c >= 0) atomicAdd(&s_start[c + 1], 1);
    }
    __syncthreads();
    {                                          // s_start[c + 1] = the end of cell c
        const int lane = tid & 63, wv = tid >> 6, c0 = 1 + kGridCpt * tid;
        int cnt[kGridCpt];
        int v = 0;
#pragma unroll
        for (int k = 0; k < kGridCpt; k++) { cnt[k] = s_start[c0 + k]; v += cnt[k]; }
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(v, o, 64);
            if (lane >= o) v += y;
        }
        if (lane == 63) s_wsum[wv] = v;
        __syncthreads();
        int end = v;
        for (int w = 0; w < wv; w++) end += s_wsum[w];
#pragma unroll
        for (int k = kGridCpt - 1; k >= 0; k--) { s_start[c0 + k] = end; end -= cnt[k]; }
    }
    __syncthreads();
    for (int c = tid; c < COEB_GRID_CELLS; c += kGridThreads) s_cur[c] = s_start[c];
    __syncthreads();
    for (int i = tid; i < n; i += kGridThreads) {
        const int c = cell_of(i);
        if (c >= 0) s_sort[atomicAdd(&s_cur[c], 1)] = i;
    }
    __syncthreads();
    for (int c = tid; c < COEB_GRID_CELLS; c += kGridThreads) {
        const int b = s_start[c], e = s_start[c + 1];
        for (int x = b + 1; x < e; x++) {
            const int key = s_sort[x];
            int y = x - 1;
            while (y >= b && s_sort[y] > key) { s_sort[y + 1] = s_sort[y]; y--; }
            s_sort[y + 1] = key;
        }
    }
    __syncthreads();
    for (int c = tid; c <= COEB_GRID_CELLS; c += kGridThreads) cell[c] = s_start[c];
    const int ng = s_start[COEB_GRID_CELLS];
    for (int e = tid; e < ng; e += kGridThreads) sorted[e] = s_sort[e];
}

// ================================= k_fuse =================================
// The search of ORBmatcher::Fuse (:843-950) over (point tile, job): kFuseLanes lanes per point, every
// lane with the point's projection (:853-891) in registers.  A window spans about 2 * th * scale / 10 px
// + 1 grid columns of a few features each, so the lanes of a point take the window's columns ix0 + lane,
// ix0 + lane + kFuseLanes, .. and walk each column's CSR range [cell[ix][iy0], cell[ix][iy1 + 1]) alone.
// The CSR position of a candidate grows along GetFeaturesInArea's enumeration (ix outer, iy inner, index
// order in a cell), so the min over (dist << 16 | position) is the smallest distance and the first of
// equals in that order: the reference's strict dist < bestDist.  A candidate that fails the window, the
// level or the chi-square test is skipped before its distance is taken.  No LDS.
// The four lanes of a point repeat its projection (one double sqrt, one double log); k_fuse takes 13 us per
// launch for 10 and for 30 targets of 1000 features, the floor of a short launch, so a
// broadcast from one lane was not tried.
// Float forms: Rcw * P + tcw as cv::Mat's small gemm (float products summed left to
// right, tcw added in double); invz = 1 / z in float, x = X * invz, u = fma(fx, x, cx), ur = fma(-bf,
// invz, u); cv::norm and Mat::dot in double, the dot compared in double with 0.5 * dist3D; PredictScale's
// (float)log((double)ratio) / mfLogScaleFactor; e2 = fma(ex, ex, ey * ey), then fma(er, er, .); the float
// product e2 * invSigma2 widened for the comparison with 7.8 / 5.99.
constexpr int kFuseThreads = 256;
constexpr int kFuseLanes = 4;
constexpr int kFusePts = kFuseThreads / kFuseLanes;
static_assert(kBowMax <= 0xFFFF, "a CSR position fits the key's low half");

struct FuseArgs {
    KfdbView v;
    const uint8_t* geo; size_t geo_stride;
    const uint8_t* grid; size_t grid_stride;
    const KfdbFuseJob* jobs;
    const uint8_t* skip;
    const uint8_t* valid; const float* pos; const float* nrm; const float* maxd; const float* mind; const uint8_t* desc;
    const float* inv_sigma2;    // [COEB_MAXL] mvInvLevelSigma2
    MatchCam cam;
    float th;
    int* best_idx; int* best_dist;
};

__global__ __launch_bounds__(kFuseThreads) void k_fuse(FuseArgs a)
{
    const KfdbFuseJob* jb = a.jobs + blockIdx.y;
    const int count = jb->count;
    if ((int)blockIdx.x * kFusePts >= count) return;               // workgroup-uniform
    const int pi = blockIdx.x * kFusePts + threadIdx.x / kFuseLanes, gl = threadIdx.x & (kFuseLanes - 1);
    const bool live = pi < count;
    const int i = jb->first + pi, slot = jb->slot;
    const MatchCam& cam = a.cam;
    const int* cell = reinterpret_cast<const int*>(a.grid + slot * a.grid_stride);
    const int* sorted = cell + COEB_GRID_CELLS + 1;
    uint32_t key = 0xFFFFFFFFu;
    bool go = live && a.valid[i] && !(jb->skip_off >= 0 && a.skip[jb->skip_off + pi]);
    float u = 0.f, v = 0.f, ur = 0.f, radius = 0.f;
    int lvl = 0;
    if (go) {
        const float* P = a.pos + (int64_t)i * 3;
        float Pc[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {                               // Rcw*p3Dw + tcw (:854)
            float t = jb->Rcw[k * 3 + 0] * P[0] + jb->Rcw[k * 3 + 1] * P[1];
            t = t + jb->Rcw[k * 3 + 2] * P[2];
            Pc[k] = (float)((double)t + (double)jb->tcw[k]);
        }
        go = !(Pc[2] < 0.0f);                                       // :857
        if (go) {
            const float invz = 1.0f / Pc[2];
            const float x = Pc[0] * invz, y = Pc[1] * invz;
            u = __builtin_fmaf(cam.fx, x, cam.cx);
            v = __builtin_fmaf(cam.fy, y, cam.cy);
            go = u >= cam.min_x && u < cam.max_x && v >= cam.min_y && v < cam.max_y;   // IsInImage (:868)
            ur = __builtin_fmaf(-cam.bf, invz, u);
        }
        if (go) {
            const float PO[3] = {P[0] - jb->Ow[0], P[1] - jb->Ow[1], P[2] - jb->Ow[2]};
            const float dist3D = (float)norm3(PO);
            const float maxd = a.maxd[i], mind = a.mind[i];
            go = !(dist3D < 0.8f * mind || dist3D > 1.2f * maxd);   // :879
            if (go) {
                const float* Pn = a.nrm + (int64_t)i * 3;
                double dot = 0.0;
                dot += (double)PO[0] * (double)Pn[0];
                dot += (double)PO[1] * (double)Pn[1];
                dot += (double)PO[2] * (double)Pn[2];
                go = !(dot < 0.5 * (double)dist3D);                 // :885
                if (go) {
                    const float ratio = maxd / dist3D;              // PredictScale (MapPoint.cc:385-400)
                    const int s = (int)ceilf((float)log((double)ratio) / cam.log_sf);
                    lvl = s < 0 ? 0 : (s >= cam.nlevels ? cam.nlevels - 1 : s);
                    radius = a.th * cam.scale[lvl];
                }
            }
        }
    }
    if (go) {
        // KeyFrame::GetFeaturesInArea (KeyFrame.cc:569-608); its four early returns leave the key as it is
        const int x0 = max(0, (int)floorf(((u - cam.min_x) - radius) * cam.grid_inv_w));
        const int x1 = min(COEB_GRID_COLS - 1, (int)ceilf(((u - cam.min_x) + radius) * cam.grid_inv_w));
        const int y0 = max(0, (int)floorf(((v - cam.min_y) - radius) * cam.grid_inv_h));
        const int y1 = min(COEB_GRID_ROWS - 1, (int)ceilf(((v - cam.min_y) + radius) * cam.grid_inv_h));
        if (x0 < COEB_GRID_COLS && x1 >= 0 && y0 < COEB_GRID_ROWS && y1 >= 0) {
            const KfdbGeo* geo = reinterpret_cast<const KfdbGeo*>(a.geo + slot * a.geo_stride);
            const uint8_t* kdesc = a.v.desc(slot);
            uint32_t q[8];
            {
                const uint4* d = reinterpret_cast<const uint4*>(a.desc + (int64_t)i * 32);
                const uint4 d0 = d[0], d1 = d[1];
                q[0] = d0.x; q[1] = d0.y; q[2] = d0.z; q[3] = d0.w;
                q[4] = d1.x; q[5] = d1.y; q[6] = d1.z; q[7] = d1.w;
            }
            for (int ix = x0 + gl; ix <= x1; ix += kFuseLanes) {
                const int c0 = cell[ix * COEB_GRID_ROWS + y0], c1 = cell[ix * COEB_GRID_ROWS + y1 + 1];
                for (int e = c0; e < c1; e++) {
                    const int idx = sorted[e];
                    const KfdbGeo g = geo[idx];
                    const float distx = g.x - u, disty = g.y - v;
                    if (!(fabsf(distx) < radius && fabsf(disty) < radius)) continue;
                    if (g.octave < lvl - 1 || g.octave > lvl) continue;             // :912
                    const float ex = u - g.x, ey = v - g.y;
                    float e2 = __builtin_fmaf(ex, ex, ey * ey);
                    if (g.u_right >= 0) {
                        const float er = ur - g.u_right;
                        e2 = __builtin_fmaf(er, er, e2);
                        if ((double)(e2 * a.inv_sigma2[g.octave]) > 7.8) continue;
                    } else if ((double)(e2 * a.inv_sigma2[g.octave]) > 5.99) {
                        continue;
                    }
                    uint32_t c[8];
                    const uint4* d = reinterpret_cast<const uint4*>(kdesc + (int64_t)idx * 32);
                    const uint4 d0 = d[0], d1 = d[1];
                    c[0] = d0.x; c[1] = d0.y; c[2] = d0.z; c[3] = d0.w;
                    c[4] = d1.x; c[5] = d1.y; c[6] = d1.z; c[7] = d1.w;
                    key = min(key, ((uint32_t)hamming32(q, c) << 16) | (uint32_t)e);
                }
            }
        }
    }
#pragma unroll
    for (int x = 1; x < kFuseLanes; x <<= 1) key = min(key, (uint32_t)__shfl_xor((int)key, x));
    if (live && gl == 0) {
        int bd = 256, bi = -1;
        if (key != 0xFFFFFFFFu && (key >> 16) < 256u) {             // dist < bestDist from 256 (:902, :945)
            bd = (int)(key >> 16);
            bi = sorted[key & 0xFFFFu];
        }
        const int o = jb->out_off + pi;
        a.best_dist[o] = bd;
        a.best_idx[o] = bd <= TH_LOW ? bi : -1;
    }
}

size_t slot_stride(int mf) { return ((size_t)mf * 48 + (size_t)csr_ints(mf) * 4 + 255) & ~(size_t)255; }

int db_err(coeb_kfdb* db, const char* what)
{
    return set_err(db ? db->c : nullptr, COEB_EINVAL, std::string(what));
}

// the one free list: every slab of the set released, the strides kept
void free_slabs(KfdbSlabs& sl)
{
    for (KfdbSlab& a : sl) {
        if (a.p) (void)hipFree(a.p);
        a.p = nullptr;
    }
}

// every slab of the set that is in use allocated for cap slots; all or (freed again) none
hipError_t alloc_slabs(KfdbSlabs& sl, int cap)
{
    for (KfdbSlab& a : sl) {
        const hipError_t e = a.stride ? hipMalloc(&a.p, (size_t)cap * a.stride) : hipSuccess;
        if (e != hipSuccess) {
            a.p = nullptr;
            free_slabs(sl);
            return e;
        }
    }
    return hipSuccess;
}

// a (geo or grid) exists afterwards, slot_bytes per slot rounded up to 256: allocated by the first call that needs it
int lazy_slab(coeb_kfdb* db, KfdbSlab& a, size_t slot_bytes, const char* what)
{
    if (a.p) return 0;
    a.stride = (slot_bytes + 255) & ~(size_t)255;
    const hipError_t e = hipMalloc(&a.p, (size_t)db->cap * a.stride);
    if (e == hipSuccess) return 0;
    a = KfdbSlab{};
    return set_err(db->c, COEB_ENOMEM, std::string("hipMalloc kfdb ") + what + ": " + hipGetErrorString(e));
}

// grow()'s copies: meta cleared, then the first nslots slots of every slab, device to device
int copy_slots(coeb_ctx* c, const KfdbSlabs& from, const KfdbSlabs& to, int nslots, int ncap, hipStream_t s)
{
    HIP_TRY(c, hipMemsetAsync(to[kMeta].p, 0, (size_t)ncap * to[kMeta].stride, s));
    for (int k = 0; k < kNumSlabs; k++) {
        const KfdbSlab &a = to[k], &o = from[k];
        if (a.p && nslots) HIP_TRY(c, hipMemcpyAsync(a.p, o.p, (size_t)nslots * a.stride, hipMemcpyDeviceToDevice, s));
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    return 0;
}

// the storage holds at least `want` slots afterwards: doubled, copied device to device.  The new set is
// a local until the copies have completed, so every return before the swap frees it.
int grow(coeb_kfdb* db, int want)
{
    coeb_ctx* c = db->c;
    if (want <= db->cap) return 0;
    int ncap = std::max(db->cap, 1);
    while (ncap < want) ncap *= 2;
    hipStream_t s = main_stream(c);
    KfdbSlabs nw = db->sl;              // the strides
    for (KfdbSlab& a : nw) a.p = nullptr;
    const hipError_t e = alloc_slabs(nw, ncap);
    if (e != hipSuccess) return set_err(c, COEB_ENOMEM, std::string("hipMalloc kfdb: ") + hipGetErrorString(e));
    if (const int rc = copy_slots(c, db->sl, nw, db->nslots, ncap, s)) {
        free_slabs(nw);
        return rc;
    }
    free_slabs(db->sl);
    db->sl = nw;
    db->cap = ncap;
    db->grid_rec.resize(ncap, KfdbGridRec{});
    db->used.resize(ncap, 0); db->has_geo.resize(ncap, 0); db->n.resize(ncap, 0); db->nd.resize(ncap, 0); db->seq.resize(ncap, 0);
    db->has_st.resize(ncap, 0); db->st_conflict.resize(ncap, 0); db->is_stereo.resize(ncap); db->depth_pos.resize(ncap);
    return 0;
}

void release_device(coeb_kfdb* db)
{
    free_slabs(db->sl);
    db->cap = db->nslots = db->nkf = 0;
}

}  // namespace

// coeb_destroy: the databases still alive lose their device memory and their context
void kfdb_release_all(coeb_ctx* c)
{
    for (coeb_kfdb* db : c->kfdbs) {
        release_device(db);
        db->c = nullptr;
    }
    c->kfdbs.clear();
}

extern "C" {

int coeb_kfdb_create(coeb_ctx* c, int max_features, int initial_slots, coeb_kfdb** out)
{
    if (out) *out = nullptr;
    if (!c || !out || max_features < 1 || max_features > kBowMax || initial_slots < 1)
        return set_err(c, COEB_EINVAL, "coeb_kfdb_create: invalid arguments");
    (void)hipSetDevice(c->device);
    coeb_kfdb* db = new coeb_kfdb;
    db->c = c;
    db->mf = max_features;
    db->sl[kSlab].stride = slot_stride(max_features);
    db->sl[kMeta].stride = 16;
    const int rc = grow(db, initial_slots);
    if (rc) { delete db; return rc; }
    c->kfdbs.push_back(db);
    *out = db;
    return COEB_OK;
}

void coeb_kfdb_destroy(coeb_kfdb* db)
{
    if (!db) return;
    if (db->c) {
        coeb_ctx* c = db->c;
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(main_stream(c));
        release_device(db);
        c->kfdbs.erase(std::remove(c->kfdbs.begin(), c->kfdbs.end(), db), c->kfdbs.end());
    }
    delete db;
}

int coeb_kfdb_add(coeb_kfdb* db, const coeb_kfdb_keyframe* kf, int* slot_out)
{
    if (!db || !db->c || !kf || !slot_out) return db_err(db, "coeb_kfdb_add: invalid arguments");
    coeb_ctx* c = db->c;
    const int n = kf->n, nw = kf->nw, mf = db->mf;
    if (n < 0 || nw < 0 || n > mf || nw > mf) return db_err(db, "coeb_kfdb_add: n or nw outside 0..max_features");
    if ((n && (!kf->descriptor || !kf->node_id || !kf->angle)) || (nw && (!kf->bow_word || !kf->bow_value)))
        return db_err(db, "coeb_kfdb_add: missing keyframe arrays");
    if (!kfdb_words_ascending(kf->bow_word, nw)) return db_err(db, "coeb_kfdb_add: bow_word is not strictly ascending");
    (void)hipSetDevice(c->device);
    int slot = 0;
    while (slot < db->nslots && db->used[slot]) slot++;           // lowest free slot first
    int rc;
    if ((rc = grow(db, slot + 1))) return rc;
    hipStream_t s = main_stream(c);
    Pack pk;
    const size_t o_val = pk.add(kf->bow_value, (size_t)nw * 8), o_word = pk.add(kf->bow_word, (size_t)nw * 4);
    const size_t o_ang = pk.add(kf->angle, (size_t)n * 4), o_desc = pk.add(kf->descriptor, (size_t)n * 32);
    const size_t o_node = pk.add(kf->node_id, (size_t)n * 4);
    uint8_t* dbase;
    if ((rc = stage_in(c, pk, &dbase, s))) return rc;
    const KfdbView v = db->view();
    StoreArgs sa;
    sa.seg[0] = StoreSeg{(const uint32_t*)(dbase + o_val), (uint32_t*)v.value(slot), nw * 2};
    sa.seg[1] = StoreSeg{(const uint32_t*)(dbase + o_word), (uint32_t*)v.word(slot), nw};
    sa.seg[2] = StoreSeg{(const uint32_t*)(dbase + o_ang), (uint32_t*)v.angle(slot), n};
    sa.seg[3] = StoreSeg{(const uint32_t*)(dbase + o_desc), (uint32_t*)v.desc(slot), n * 8};
    sa.meta = v.meta + slot * 4; sa.n = n; sa.nw = nw;
    prof_begin(&c->hook, "k_kfdb_store", s);
    hipLaunchKernelGGL(k_kfdb_store, dim3(std::max(1, (n * 8 + kDbThreads - 1) / kDbThreads)), dim3(kDbThreads), 0, s, sa);
    prof_end(&c->hook, s);
    CsrArgs ca{};
    ca.side[0] = CsrSide{(const int*)(dbase + o_node), nullptr, n, v.csr(slot)};
    launch_bow_csr(c, ca, 1, s);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->pin, v.csr(slot), 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    db->used[slot] = 1;
    db->drop(slot);
    db->n[slot] = n;
    db->nd[slot] = reinterpret_cast<const int32_t*>(c->pin)[0];
    db->seq[slot] = db->next_seq++;
    db->nslots = std::max(db->nslots, slot + 1);
    db->nkf++;
    *slot_out = slot;
    return COEB_OK;
}

int coeb_kfdb_erase(coeb_kfdb* db, int slot)
{
    if (!db || !db->c) return db_err(db, "coeb_kfdb_erase: invalid arguments");
    if (slot < 0 || slot >= db->nslots || !db->used[slot]) return db_err(db, "coeb_kfdb_erase: no keyframe in that slot");
    coeb_ctx* c = db->c;
    (void)hipSetDevice(c->device);
    HIP_TRY(c, hipMemsetAsync(db->sl[kMeta].p + slot * 16, 0, 16, main_stream(c)));
    db->used[slot] = 0;
    db->drop(slot);
    db->n[slot] = db->nd[slot] = 0;
    db->nkf--;
    return COEB_OK;
}

int coeb_kfdb_clear(coeb_kfdb* db)
{
    if (!db || !db->c) return db_err(db, "coeb_kfdb_clear: invalid arguments");
    coeb_ctx* c = db->c;
    (void)hipSetDevice(c->device);
    HIP_TRY(c, hipMemsetAsync(db->sl[kMeta].p, 0, (size_t)db->cap * 16, main_stream(c)));
    std::fill(db->used.begin(), db->used.end(), 0);
    for (int sl = 0; sl < db->cap; sl++) db->drop(sl);
    std::fill(db->n.begin(), db->n.end(), 0);
    std::fill(db->nd.begin(), db->nd.end(), 0);
    db->nslots = db->nkf = 0;
    return COEB_OK;
}

int coeb_kfdb_size(const coeb_kfdb* db, int* nkeyframes, int* nslots)
{
    if (!db) return set_err(nullptr, COEB_EINVAL, "coeb_kfdb_size: invalid arguments");
    if (nkeyframes) *nkeyframes = db->nkf;
    if (nslots) *nslots = db->nslots;
    return COEB_OK;
}

int coeb_kfdb_query(coeb_kfdb* db, const int32_t* word, const double* value, int nw, int32_t* common, float* score,
                    int32_t* order, int* n_sharing, int* max_common, int* min_common)
{
    if (!db || !db->c || !n_sharing || !max_common || !min_common || nw < 0 || (nw && (!word || !value)))
        return db_err(db, "coeb_kfdb_query: invalid arguments");
    coeb_ctx* c = db->c;
    const int ns = db->nslots;
    if (ns && (!common || !score || !order)) return db_err(db, "coeb_kfdb_query: missing output arrays");
    if (nw > db->mf) return db_err(db, "coeb_kfdb_query: more query words than max_features");
    if (!kfdb_words_ascending(word, nw)) return db_err(db, "coeb_kfdb_query: word is not strictly ascending");
    *n_sharing = *max_common = *min_common = 0;
    if (!ns || !nw || !db->nkf) {
        for (int i = 0; i < ns; i++) { common[i] = 0; score[i] = -1.0f; }
        return COEB_OK;
    }
    (void)hipSetDevice(c->device);
    hipStream_t s = main_stream(c);
    Staged st;
    const size_t o_val = st.add(value, (size_t)nw * 8), o_word = st.add(word, (size_t)nw * 4);
    // results: the header {max, min common words, 0, 0} with its initial value, then what the kernels write per slot
    const size_t o_hdr = st.fill(0, 16);
    const size_t o_com = st.take((size_t)ns * 4), o_first = st.take((size_t)ns * 4), o_score = st.take((size_t)ns * 4);
    int rc;
    if ((rc = st.stage(c, s, false))) return rc;
    const KfdbView v = db->view();
    const dim3 grid((ns + kDbWaves - 1) / kDbWaves);
    prof_begin(&c->hook, "k_kfdb_common", s);
    hipLaunchKernelGGL(k_kfdb_common, grid, dim3(kDbThreads), 0, s, v, ns, st.dev<int>(o_word), nw, st.dev<int>(o_hdr),
                       st.dev<int>(o_com), st.dev<int>(o_first));
    prof_end(&c->hook, s);
    prof_begin(&c->hook, "k_kfdb_score", s);
    hipLaunchKernelGGL(k_kfdb_score, grid, dim3(kDbThreads), 0, s, v, ns, st.dev<int>(o_word), st.dev<double>(o_val),
                       nw, st.dev<int>(o_hdr), st.dev<int>(o_com), st.dev<float>(o_score));
    prof_end(&c->hook, s);
    HIP_TRY(c, hipGetLastError());
    if ((rc = st.finish(c, s, o_hdr, st.end(), false))) return rc;
    *max_common = st.host<int32_t>(o_hdr)[0];
    *min_common = st.host<int32_t>(o_hdr)[1];
    memcpy(common, st.host<int32_t>(o_com), (size_t)ns * 4);
    memcpy(score, st.host<float>(o_score), (size_t)ns * 4);
    *n_sharing = kfdb_sharing_order(common, st.host<int32_t>(o_first), db->seq.data(), ns, order);
    return COEB_OK;
}

int coeb_match_bow_kfdb(coeb_kfdb* db, const int32_t* slots, int ncand, const uint8_t* const* valid,
                        const coeb_bow_frame* cur, float nnratio, int check_orientation, int32_t* match_out,
                        int32_t* nmatches)
{
    if (!db || !db->c || !cur || ncand < 0) return db_err(db, "coeb_match_bow_kfdb: invalid arguments");
    coeb_ctx* c = db->c;
    if (ncand > kMaxCand) return db_err(db, "coeb_match_bow_kfdb: more than 256 candidates");
    const int n = cur->n;
    if (n < 0 || n > kBowMax) return db_err(db, "coeb_match_bow_kfdb: frame size outside 0..4095");
    if (ncand == 0) return COEB_OK;
    if (!slots || !valid || !nmatches || (n && (!cur->descriptor || !cur->node_id || !cur->angle || !match_out)))
        return db_err(db, "coeb_match_bow_kfdb: missing arrays");
    int max_nd = 0;
    for (int j = 0; j < ncand; j++) {
        const int sl = slots[j];
        if (sl < 0 || sl >= db->nslots || !db->used[sl]) return db_err(db, "coeb_match_bow_kfdb: no keyframe in a candidate's slot");
        if (db->n[sl] && !valid[j]) return db_err(db, "coeb_match_bow_kfdb: missing valid mask");
        max_nd = std::max(max_nd, db->nd[sl]);
    }
    (void)hipSetDevice(c->device);
    const int cs = std::max(n, 1);
    const size_t nout = (size_t)ncand * cs + ncand;
    BowBufs& bw = c->bow;
    int rc;
    if ((rc = ensure(c, bw.m_csr, (size_t)csr_ints(n))) || (rc = ensure(c, bw.m_aux, (size_t)ncand * (cs + 32)))) return rc;
    hipStream_t s = main_stream(c);
    Staged st;
    std::vector<int32_t> cand((size_t)ncand * 2);
    const size_t o_cand = st.add(cand.data(), cand.size() * 4);
    const size_t o_cd = st.add(cur->descriptor, (size_t)n * 32), o_cn = st.add(cur->node_id, (size_t)n * 4);
    const size_t o_ca = st.add(cur->angle, (size_t)n * 4);
    for (int j = 0; j < ncand; j++) {
        cand[2 * j] = slots[j];
        cand[2 * j + 1] = (int32_t)st.add(valid[j], (size_t)db->n[slots[j]]);
    }
    const size_t o_m = st.take(nout * 4);           // the match rows, then the counts: k_bow_csr clears them in one run
    if ((rc = st.stage(c, s, false))) return rc;
    int* csr_c = bw.m_csr.p;
    DbMatch a;
    a.v = db->view();
    a.cand = st.dev<int>(o_cand);
    a.stage = st.dbase;
    a.cur = BowSide{st.dev<uint8_t>(o_cd), st.dev<float>(o_ca), csr_c, n};
    a.nnratio = nnratio; a.check_ori = check_orientation ? 1 : 0; a.cs = cs;
    a.match = st.dev<int>(o_m); a.nm = a.match + (size_t)ncand * cs;
    a.bin = bw.m_aux.p; a.hist = a.bin + (size_t)ncand * cs;
    CsrArgs ca{};
    ca.side[0] = CsrSide{st.dev<int>(o_cn), nullptr, n, csr_c};
    ca.clear_m1 = a.match; ca.clear_n = (int)nout;
    ca.clear_0 = a.bin; ca.clear_0n = ncand * (cs + 32);
    launch_bow_csr(c, ca, 1, s);
    if (n && max_nd) {
        prof_begin(&c->hook, "k_match_bow_db", s);
        hipLaunchKernelGGL(k_match_bow_db, dim3((max_nd + kBowWaves - 1) / kBowWaves, ncand), dim3(kBowThreads), 0, s, a);
        prof_end(&c->hook, s);
    }
    prof_begin(&c->hook, "k_bow_rot_db", s);
    hipLaunchKernelGGL(k_bow_rot_db, dim3(ncand), dim3(kCsrThreads), 0, s, a);
    prof_end(&c->hook, s);
    HIP_TRY(c, hipGetLastError());
    if ((rc = st.finish(c, s, o_m, st.end(), false))) return rc;
    const int32_t* hout = st.host<int32_t>(o_m);
    for (int j = 0; j < ncand && n; j++) memcpy(match_out + (size_t)j * n, hout + (size_t)j * cs, (size_t)n * 4);
    memcpy(nmatches, hout + (size_t)ncand * cs, (size_t)ncand * 4);
    return COEB_OK;
}

int coeb_kfdb_set_geometry(coeb_kfdb* db, int slot, const coeb_keypoint* keys_un, const float* u_right)
{
    if (!db || !db->c) return db_err(db, "coeb_kfdb_set_geometry: invalid arguments");
    if (slot < 0 || slot >= db->nslots || !db->used[slot]) return db_err(db, "coeb_kfdb_set_geometry: no keyframe in that slot");
    coeb_ctx* c = db->c;
    const int n = db->n[slot];
    if (n && (!keys_un || !u_right)) return db_err(db, "coeb_kfdb_set_geometry: missing keyframe arrays");
    (void)hipSetDevice(c->device);
    int rc;
    if ((rc = pinned(c, (size_t)n * sizeof(KfdbGeo)))) return rc;
    if (!kfdb_pack_geometry(keys_un, u_right, n, c->tab.nlevels, reinterpret_cast<KfdbGeo*>(c->pin)))
        return db_err(db, "coeb_kfdb_set_geometry: keypoint octave outside the pyramid");
    KfdbSlab& geo = db->sl[kGeo];
    if ((rc = lazy_slab(db, geo, (size_t)db->mf * sizeof(KfdbGeo), "geometry"))) return rc;
    if (n) {
        hipStream_t s = main_stream(c);
        HIP_TRY(c, hipMemcpyAsync(geo.p + slot * geo.stride, c->pin, (size_t)n * sizeof(KfdbGeo), hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipStreamSynchronize(s));       // the page-locked buffer is the next call's
    }
    db->has_geo[slot] = 1;
    db->grid_rec[slot].built = 0;
    // host-only bookkeeping for coeb_kfdb_create_new_map_points' refusal of a stereo feature without depth,
    // whichever of this call and coeb_kfdb_set_stereo comes last; the slab and every other call are as before
    db->is_stereo[slot].resize((size_t)n);
    for (int i = 0; i < n; i++) db->is_stereo[slot][i] = u_right[i] >= 0;
    db->note_conflict(slot);
    return COEB_OK;
}

int coeb_kfdb_set_stereo(coeb_kfdb* db, int slot, const float* key_xy, const float* depth)
{
    if (!db || !db->c) return db_err(db, "coeb_kfdb_set_stereo: invalid arguments");
    if (slot < 0 || slot >= db->nslots || !db->used[slot]) return db_err(db, "coeb_kfdb_set_stereo: no keyframe in that slot");
    coeb_ctx* c = db->c;
    const int n = db->n[slot];
    if (n && (!key_xy || !depth)) return db_err(db, "coeb_kfdb_set_stereo: missing keyframe arrays");
    (void)hipSetDevice(c->device);
    int rc;
    if ((rc = pinned(c, (size_t)n * sizeof(KfdbStereo)))) return rc;
    std::vector<uint8_t> pos((size_t)n);
    if (!kfdb_pack_stereo(key_xy, depth, n, reinterpret_cast<KfdbStereo*>(c->pin), pos.data()))
        return db_err(db, "coeb_kfdb_set_stereo: a keypoint or depth entry is not finite");
    KfdbSlab& st = db->sl[kStereo];
    if ((rc = lazy_slab(db, st, (size_t)db->mf * sizeof(KfdbStereo), "stereo data"))) return rc;
    if (n) {
        hipStream_t s = main_stream(c);
        HIP_TRY(c, hipMemcpyAsync(st.p + slot * st.stride, c->pin, (size_t)n * sizeof(KfdbStereo), hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipStreamSynchronize(s));       // the page-locked buffer is the next call's
    }
    db->has_st[slot] = 1;
    db->depth_pos[slot].swap(pos);
    db->note_conflict(slot);
    return COEB_OK;
}

// Uploaded: both masks, the slot table, F12, the epipoles, the level tables, the zeroed histograms and
// the match rows as -1.  Copied back: the match rows and the counts.
int coeb_kfdb_search_triangulation(coeb_kfdb* db, int slot1, const uint8_t* has_mp1, const int32_t* slots2, int nnb,
                                   const uint8_t* const* has_mp2, const float* F12, const float* epipole,
                                   int only_stereo, int check_orientation, int32_t* match_out, int32_t* nmatches)
{
    const std::string w("coeb_kfdb_search_triangulation: ");
    if (!db || !db->c) return db_err(db, (w + "invalid arguments").c_str());
    coeb_ctx* c = db->c;
    const char* why = kfdb_tri_check(db->used.data(), db->has_geo.data(), db->n.data(), db->nslots, slot1, has_mp1, slots2,
                                     nnb, has_mp2, F12, epipole, match_out, nmatches);
    if (why) return db_err(db, (w + why).c_str());
    if (nnb == 0) return COEB_OK;
    const int n1 = db->n[slot1];
    if (n1 == 0) {
        memset(nmatches, 0, (size_t)nnb * 4);
        return COEB_OK;
    }
    (void)hipSetDevice(c->device);
    hipStream_t s = main_stream(c);
    std::vector<uint8_t> masks;
    std::vector<int32_t> tab;
    kfdb_tri_pack(db->n.data(), slots2, nnb, has_mp2, masks, tab);
    const size_t rows = (size_t)nnb * n1;
    Staged st;
    const size_t o_h1 = st.add(has_mp1, (size_t)n1), o_mk = st.add(masks.data(), masks.size());
    const size_t o_tab = st.add(tab.data(), tab.size() * 4), o_F = st.add(F12, (size_t)nnb * 36);
    const size_t o_e = st.add(epipole, (size_t)nnb * 8);
    const size_t o_sc = st.add(c->tab.scale, sizeof(float) * COEB_MAXL), o_sg = st.add(c->tab.sigma2, sizeof(float) * COEB_MAXL);
    const size_t o_hist = st.fill(0, (size_t)nnb * 32 * 4);
    // results: the match rows with their initial value, the counts; then scratch
    const size_t o_m = st.fill(0xFF, rows * 4), o_nm = st.take((size_t)nnb * 4);
    const size_t back_end = st.end();
    const size_t o_bin = st.take(rows * 4);
    int rc;
    if ((rc = st.stage(c, s, false))) return rc;
    TriArgs a;
    a.v = db->view(); a.geo = db->sl[kGeo].p; a.geo_stride = db->sl[kGeo].stride; a.slot1 = slot1;
    a.has1 = st.dev<uint8_t>(o_h1); a.tab = st.dev<int>(o_tab); a.masks = st.dev<uint8_t>(o_mk);
    a.F = st.dev<float>(o_F); a.epi = st.dev<float>(o_e); a.scale = st.dev<float>(o_sc); a.sigma2 = st.dev<float>(o_sg);
    a.only_stereo = only_stereo ? 1 : 0; a.check_ori = check_orientation ? 1 : 0; a.cs = n1;
    a.match = st.dev<int>(o_m); a.bin = st.dev<int>(o_bin); a.hist = st.dev<int>(o_hist); a.nm = st.dev<int>(o_nm);
    if (db->nd[slot1]) {
        prof_begin(&c->hook, "k_tri_match", s);
        hipLaunchKernelGGL(k_tri_match, dim3(db->nd[slot1], nnb), dim3(kTriThreads), 0, s, a);
        prof_end(&c->hook, s);
    }
    prof_begin(&c->hook, "k_tri_rot", s);
    hipLaunchKernelGGL(k_tri_rot, dim3(nnb), dim3(kCsrThreads), 0, s, a, n1);
    prof_end(&c->hook, s);
    HIP_TRY(c, hipGetLastError());
    if ((rc = st.finish(c, s, o_m, back_end, false))) return rc;
    memcpy(match_out, st.host<int32_t>(o_m), rows * 4);
    memcpy(nmatches, st.host<int32_t>(o_nm), (size_t)nnb * 4);
    return COEB_OK;
}

// Uploaded: what coeb_kfdb_search_triangulation uploads without the histograms, the views, first_ok as
// INT_MAX.  Copied back: the match rows, first_ok, x3d and the status bytes, one range.
int coeb_kfdb_create_new_map_points(coeb_kfdb* db, int slot1, const coeb_kf_view* view1, const uint8_t* has_mp1,
                                    const int32_t* slots2, int nnb, const coeb_kf_view* views2,
                                    const uint8_t* const* has_mp2, const float* F12, const float* epipole,
                                    int only_stereo, int32_t* match_out, int8_t* status, float* x3d,
                                    int32_t* first_ok, int32_t* nmatches)
{
    const std::string w("coeb_kfdb_create_new_map_points: ");
    if (!db || !db->c) return db_err(db, (w + "invalid arguments").c_str());
    coeb_ctx* c = db->c;
    const char* why = kfdb_newpts_check(db->used.data(), db->has_geo.data(), db->has_st.data(), db->st_conflict.data(),
                                        db->n.data(), db->nslots, slot1, view1, has_mp1, slots2, nnb, views2, has_mp2, F12,
                                        epipole, match_out, status, x3d, first_ok, nmatches);
    if (why) return db_err(db, (w + why).c_str());
    const int n1 = db->n[slot1];
    for (int i = 0; i < n1; i++) first_ok[i] = -1;
    if (nnb == 0) return COEB_OK;
    if (n1 == 0) {
        memset(nmatches, 0, (size_t)nnb * 4);
        return COEB_OK;
    }
    (void)hipSetDevice(c->device);
    hipStream_t s = main_stream(c);
    std::vector<uint8_t> masks;
    std::vector<int32_t> tab;
    kfdb_tri_pack(db->n.data(), slots2, nnb, has_mp2, masks, tab);
    const size_t rows = (size_t)nnb * n1;
    const std::vector<int32_t> none((size_t)n1, INT_MAX);
    std::vector<coeb_kf_view> views(1, *view1);         // keyframe 1, then the neighbours
    views.insert(views.end(), views2, views2 + nnb);
    Staged st;
    const size_t o_h1 = st.add(has_mp1, (size_t)n1), o_mk = st.add(masks.data(), masks.size());
    const size_t o_tab = st.add(tab.data(), tab.size() * 4), o_F = st.add(F12, (size_t)nnb * 36);
    const size_t o_e = st.add(epipole, (size_t)nnb * 8);
    const size_t o_sc = st.add(c->tab.scale, sizeof(float) * COEB_MAXL), o_sg = st.add(c->tab.sigma2, sizeof(float) * COEB_MAXL);
    const size_t o_v1 = st.add(views.data(), views.size() * sizeof(coeb_kf_view));
    // results: the match rows and first_ok with their initial values, then what k_tri_points writes
    const size_t o_m = st.fill(0xFF, rows * 4), o_first = st.add(none.data(), (size_t)n1 * 4);
    const size_t o_x = st.take(rows * 12), o_st = st.take(rows);
    const size_t back_end = st.end();
    int rc;
    if ((rc = st.stage(c, s, false))) return rc;
    TriArgs a;
    a.v = db->view(); a.geo = db->sl[kGeo].p; a.geo_stride = db->sl[kGeo].stride; a.slot1 = slot1;
    a.has1 = st.dev<uint8_t>(o_h1); a.tab = st.dev<int>(o_tab); a.masks = st.dev<uint8_t>(o_mk);
    a.F = st.dev<float>(o_F); a.epi = st.dev<float>(o_e); a.scale = st.dev<float>(o_sc); a.sigma2 = st.dev<float>(o_sg);
    a.only_stereo = only_stereo ? 1 : 0; a.check_ori = 0; a.cs = n1;
    a.match = st.dev<int>(o_m); a.bin = nullptr; a.hist = nullptr; a.nm = nullptr;     // read under check_ori alone
    if (db->nd[slot1]) {
        prof_begin(&c->hook, "k_tri_match", s);
        hipLaunchKernelGGL(k_tri_match, dim3(db->nd[slot1], nnb), dim3(kTriThreads), 0, s, a);
        prof_end(&c->hook, s);
    }
    PtsArgs p;
    p.geo = a.geo; p.geo_stride = a.geo_stride; p.st = db->sl[kStereo].p; p.st_stride = db->sl[kStereo].stride;
    p.slot1 = slot1; p.tab = a.tab; p.view = st.dev<coeb_kf_view>(o_v1); p.scale = a.scale; p.sigma2 = a.sigma2;
    p.ratio_factor = 1.5f * (float)c->tab.scale_factor;
    p.n1 = n1; p.match = a.match;
    p.status = st.dev<int8_t>(o_st); p.x3d = st.dev<float>(o_x); p.first = st.dev<int>(o_first);
    prof_begin(&c->hook, "k_tri_points", s);
    hipLaunchKernelGGL(k_tri_points, dim3((n1 + kPtsThreads - 1) / kPtsThreads, nnb), dim3(kPtsThreads), 0, s, p);
    prof_end(&c->hook, s);
    HIP_TRY(c, hipGetLastError());
    if ((rc = st.finish(c, s, o_m, back_end, false))) return rc;
    memcpy(match_out, st.host<int32_t>(o_m), rows * 4);
    memcpy(status, st.host<int8_t>(o_st), rows);
    kfdb_newpts_unpack(match_out, status, st.host<float>(o_x), st.host<int32_t>(o_first), nnb, n1, x3d, first_ok, nmatches);
    return COEB_OK;
}

// Uploaded: the point list, the job table, the skip bytes, mvInvLevelSigma2 and the slots whose grid is
// built first.  Copied back: best_idx and best_dist, which k_fuse writes for every pair.
int coeb_kfdb_fuse_search(coeb_kfdb* db, const coeb_camera* cam, const coeb_fuse_points* pts, const coeb_fuse_job* jobs,
                          int njobs, float th, int32_t* best_idx, int32_t* best_dist)
{
    const std::string w("coeb_kfdb_fuse_search: ");
    if (!db || !db->c) return db_err(db, (w + "invalid arguments").c_str());
    coeb_ctx* c = db->c;
    int code;
    int64_t total;
    const char* why = kfdb_fuse_check(db->used.data(), db->has_geo.data(), db->nslots, cam, pts, jobs, njobs, th, best_idx,
                                      best_dist, &code, &total);
    if (why) return set_err(c, code, w + why);
    if (total == 0) return COEB_OK;
    (void)hipSetDevice(c->device);
    hipStream_t s = main_stream(c);
    int rc;
    if ((rc = lazy_slab(db, db->sl[kGrid], fuse_grid_ints(db->mf) * 4, "grids"))) return rc;
    const KfdbSlab &geo = db->sl[kGeo], &grid = db->sl[kGrid];
    std::vector<KfdbFuseJob> tab;
    std::vector<uint8_t> skip;
    std::vector<int32_t> build;
    kfdb_fuse_pack(jobs, njobs, db->grid_rec.data(), cam, tab, skip, build);
    const size_t n = (size_t)pts->n;
    int max_count = 0;
    for (const KfdbFuseJob& t : tab) max_count = std::max(max_count, t.count);
    Staged st;
    const size_t o_v = st.add(pts->valid, n), o_x = st.add(pts->world_pos, n * 12), o_nr = st.add(pts->normal, n * 12);
    const size_t o_mx = st.add(pts->max_distance, n * 4), o_mn = st.add(pts->min_distance, n * 4);
    const size_t o_d = st.add(pts->descriptor, n * 32);
    const size_t o_tab = st.add(tab.data(), tab.size() * sizeof(KfdbFuseJob)), o_sk = st.add(skip.data(), skip.size());
    const size_t o_is = st.add(c->tab.inv_sigma2, sizeof(float) * COEB_MAXL);
    const size_t o_bs = st.add(build.data(), build.size() * 4);
    const size_t o_bi = st.take((size_t)total * 4), o_bd = st.take((size_t)total * 4);
    const size_t back_end = st.end();
    if ((rc = st.stage(c, s, false))) return rc;
    const MatchCam mc = make_cam(c, cam);
    if (!build.empty()) {
        FuseGridArgs g;
        g.v = db->view(); g.geo = geo.p; g.geo_stride = geo.stride; g.grid = grid.p; g.grid_stride = grid.stride;
        g.slots = st.dev<int>(o_bs);
        g.min_x = mc.min_x; g.min_y = mc.min_y; g.inv_w = mc.grid_inv_w; g.inv_h = mc.grid_inv_h;
        prof_begin(&c->hook, "k_fuse_grid", s);
        hipLaunchKernelGGL(k_fuse_grid, dim3((unsigned)build.size()), dim3(kGridThreads), 0, s, g);
        prof_end(&c->hook, s);
    }
    FuseArgs a;
    a.v = db->view(); a.geo = geo.p; a.geo_stride = geo.stride; a.grid = grid.p; a.grid_stride = grid.stride;
    a.jobs = st.dev<KfdbFuseJob>(o_tab); a.skip = st.dev<uint8_t>(o_sk);
    a.valid = st.dev<uint8_t>(o_v); a.pos = st.dev<float>(o_x); a.nrm = st.dev<float>(o_nr);
    a.maxd = st.dev<float>(o_mx); a.mind = st.dev<float>(o_mn); a.desc = st.dev<uint8_t>(o_d);
    a.inv_sigma2 = st.dev<float>(o_is); a.cam = mc; a.th = th;
    a.best_idx = st.dev<int>(o_bi); a.best_dist = st.dev<int>(o_bd);
    prof_begin(&c->hook, "k_fuse", s);
    hipLaunchKernelGGL(k_fuse, dim3((max_count + kFusePts - 1) / kFusePts, njobs), dim3(kFuseThreads), 0, s, a);
    prof_end(&c->hook, s);
    HIP_TRY(c, hipGetLastError());
    if ((rc = st.finish(c, s, o_bi, back_end, false))) return rc;
    for (const int32_t sl : build) db->grid_rec[sl] = KfdbGridRec{1, cam->min_x, cam->max_x, cam->min_y, cam->max_y};
    memcpy(best_idx, st.host<int32_t>(o_bi), (size_t)total * 4);
    memcpy(best_dist, st.host<int32_t>(o_bd), (size_t)total * 4);
    return COEB_OK;
}

}  // extern "C"
