// coeb_kfdb.hip -- the keyframe database of Tracking::Relocalization on the device:
//   KeyFrameDatabase::add / erase / clear                src/KeyFrameDatabase.cc:40-73
//   DetectRelocalizationCandidates up to lScoreAndMatch  src/KeyFrameDatabase.cc:199-253
//                                                        (k_kfdb_common, k_kfdb_score)
//   SearchByBoW against every candidate                  src/Tracking.cc:1449-1470 (k_match_bow_db)
// What a keyframe contributes never changes after KeyFrame::ComputeBoW, so it is uploaded once
// (descriptors, angles, BowVector) and its feature-vector CSR is built once.  There is no inverted
// file: mnRelocWords of a keyframe is |words(F) & words(KF)|, counted per keyframe.  The scoring
// restates DBoW2's L1Scoring; parity against DBoW2 itself is UNPINNED.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstring>
#include <vector>

#include "coeb_bow_dev.hpp"
#include "coeb_kfdb_host.hpp"

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

struct coeb_kfdb {
    coeb_ctx* c = nullptr;          // null once the context is gone
    KfdbView v{nullptr, 0, nullptr, 0};
    int cap = 0;                    // allocated slots
    int nslots = 0;                 // one past the highest slot handed out
    int nkf = 0;
    int* q = nullptr;               // query scratch: hdr[4] {max, min}, common[cap], first[cap], score[cap]
    int64_t next_seq = 0;
    std::vector<uint8_t> used;
    std::vector<int> n, nd;         // features and feature-vector nodes per slot
    std::vector<int64_t> seq;       // insertion sequence number per slot
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

size_t slot_stride(int mf) { return ((size_t)mf * 48 + (size_t)csr_ints(mf) * 4 + 255) & ~(size_t)255; }

int db_err(coeb_kfdb* db, const char* what)
{
    return set_err(db ? db->c : nullptr, COEB_EINVAL, std::string(what));
}

// the storage holds at least `want` slots afterwards: doubled, copied device to device
int grow(coeb_kfdb* db, int want)
{
    coeb_ctx* c = db->c;
    if (want <= db->cap) return 0;
    int ncap = std::max(db->cap, 1);
    while (ncap < want) ncap *= 2;
    hipStream_t s = main_stream(c);
    uint8_t* slab = nullptr;
    int* meta = nullptr;
    int* q = nullptr;
    hipError_t e = hipMalloc(&slab, (size_t)ncap * db->v.stride);
    if (e == hipSuccess) e = hipMalloc(&meta, (size_t)ncap * 16);
    if (e == hipSuccess) e = hipMalloc(&q, (4 + 3 * (size_t)ncap) * 4);
    if (e != hipSuccess) {
        if (slab) (void)hipFree(slab);
        if (meta) (void)hipFree(meta);
        return set_err(c, COEB_ENOMEM, std::string("hipMalloc kfdb: ") + hipGetErrorString(e));
    }
    HIP_TRY(c, hipMemsetAsync(meta, 0, (size_t)ncap * 16, s));
    if (db->nslots) {
        HIP_TRY(c, hipMemcpyAsync(slab, db->v.slab, (size_t)db->nslots * db->v.stride, hipMemcpyDeviceToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(meta, db->v.meta, (size_t)db->nslots * 16, hipMemcpyDeviceToDevice, s));
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    if (db->v.slab) (void)hipFree(db->v.slab);
    if (db->v.meta) (void)hipFree(db->v.meta);
    if (db->q) (void)hipFree(db->q);
    db->v.slab = slab; db->v.meta = meta; db->q = q; db->cap = ncap;
    db->used.resize(ncap, 0); db->n.resize(ncap, 0); db->nd.resize(ncap, 0); db->seq.resize(ncap, 0);
    return 0;
}

void release_device(coeb_kfdb* db)
{
    if (db->v.slab) (void)hipFree(db->v.slab);
    if (db->v.meta) (void)hipFree(db->v.meta);
    if (db->q) (void)hipFree(db->q);
    db->v.slab = nullptr; db->v.meta = nullptr; db->q = nullptr;
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
    db->v.mf = max_features;
    db->v.stride = slot_stride(max_features);
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
    const int n = kf->n, nw = kf->nw, mf = db->v.mf;
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
    StoreArgs sa;
    sa.seg[0] = StoreSeg{(const uint32_t*)(dbase + o_val), (uint32_t*)db->v.value(slot), nw * 2};
    sa.seg[1] = StoreSeg{(const uint32_t*)(dbase + o_word), (uint32_t*)db->v.word(slot), nw};
    sa.seg[2] = StoreSeg{(const uint32_t*)(dbase + o_ang), (uint32_t*)db->v.angle(slot), n};
    sa.seg[3] = StoreSeg{(const uint32_t*)(dbase + o_desc), (uint32_t*)db->v.desc(slot), n * 8};
    sa.meta = db->v.meta + slot * 4; sa.n = n; sa.nw = nw;
    prof_begin(&c->hook, "k_kfdb_store", s);
    hipLaunchKernelGGL(k_kfdb_store, dim3(std::max(1, (n * 8 + kDbThreads - 1) / kDbThreads)), dim3(kDbThreads), 0, s, sa);
    prof_end(&c->hook, s);
    CsrArgs ca{};
    ca.side[0] = CsrSide{(const int*)(dbase + o_node), nullptr, n, db->v.csr(slot)};
    launch_bow_csr(c, ca, 1, s);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->pin, db->v.csr(slot), 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    db->used[slot] = 1;
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
    HIP_TRY(c, hipMemsetAsync(db->v.meta + slot * 4, 0, 16, main_stream(c)));
    db->used[slot] = 0;
    db->n[slot] = db->nd[slot] = 0;
    db->nkf--;
    return COEB_OK;
}

int coeb_kfdb_clear(coeb_kfdb* db)
{
    if (!db || !db->c) return db_err(db, "coeb_kfdb_clear: invalid arguments");
    coeb_ctx* c = db->c;
    (void)hipSetDevice(c->device);
    HIP_TRY(c, hipMemsetAsync(db->v.meta, 0, (size_t)db->cap * 16, main_stream(c)));
    std::fill(db->used.begin(), db->used.end(), 0);
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
    if (nw > db->v.mf) return db_err(db, "coeb_kfdb_query: more query words than max_features");
    if (!kfdb_words_ascending(word, nw)) return db_err(db, "coeb_kfdb_query: word is not strictly ascending");
    *n_sharing = *max_common = *min_common = 0;
    if (!ns || !nw || !db->nkf) {
        for (int i = 0; i < ns; i++) { common[i] = 0; score[i] = -1.0f; }
        return COEB_OK;
    }
    (void)hipSetDevice(c->device);
    hipStream_t s = main_stream(c);
    Pack pk;
    const size_t o_val = pk.add(value, (size_t)nw * 8), o_word = pk.add(word, (size_t)nw * 4);
    const size_t nout = 4 + 3 * (size_t)ns;
    uint8_t* dbase;
    int rc;
    if ((rc = pinned(c, std::max(pk.total, nout * 4))) || (rc = stage_in(c, pk, &dbase, s))) return rc;
    int* hdr = db->q;
    int* d_common = hdr + 4;
    int* d_first = d_common + ns;
    float* d_score = reinterpret_cast<float*>(d_first + ns);
    HIP_TRY(c, hipMemsetAsync(hdr, 0, 16, s));
    const dim3 grid((ns + kDbWaves - 1) / kDbWaves);
    prof_begin(&c->hook, "k_kfdb_common", s);
    hipLaunchKernelGGL(k_kfdb_common, grid, dim3(kDbThreads), 0, s, db->v, ns, (const int*)(dbase + o_word), nw, hdr,
                       d_common, d_first);
    prof_end(&c->hook, s);
    prof_begin(&c->hook, "k_kfdb_score", s);
    hipLaunchKernelGGL(k_kfdb_score, grid, dim3(kDbThreads), 0, s, db->v, ns, (const int*)(dbase + o_word),
                       (const double*)(dbase + o_val), nw, hdr, d_common, d_score);
    prof_end(&c->hook, s);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->pin, hdr, nout * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    const int32_t* h = reinterpret_cast<const int32_t*>(c->pin);
    *max_common = h[0];
    *min_common = h[1];
    memcpy(common, h + 4, (size_t)ns * 4);
    memcpy(score, h + 4 + 2 * (size_t)ns, (size_t)ns * 4);
    *n_sharing = kfdb_sharing_order(common, h + 4 + ns, db->seq.data(), ns, order);
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
    if ((rc = ensure(c, bw.m_csr, (size_t)csr_ints(n))) || (rc = ensure(c, bw.m_out, nout)) ||
        (rc = ensure(c, bw.m_aux, (size_t)ncand * (cs + 32))))
        return rc;
    hipStream_t s = main_stream(c);
    Pack pk;
    std::vector<int32_t> cand((size_t)ncand * 2);
    const size_t o_cand = pk.add(cand.data(), cand.size() * 4);
    const size_t o_cd = pk.add(cur->descriptor, (size_t)n * 32), o_cn = pk.add(cur->node_id, (size_t)n * 4);
    const size_t o_ca = pk.add(cur->angle, (size_t)n * 4);
    for (int j = 0; j < ncand; j++) {
        cand[2 * j] = slots[j];
        cand[2 * j + 1] = (int32_t)pk.add(valid[j], (size_t)db->n[slots[j]]);
    }
    uint8_t* dbase;
    if ((rc = pinned(c, std::max(pk.total, nout * 4))) || (rc = stage_in(c, pk, &dbase, s))) return rc;
    int* csr_c = bw.m_csr.p;
    DbMatch a;
    a.v = db->v;
    a.cand = (const int*)(dbase + o_cand);
    a.stage = dbase;
    a.cur = BowSide{dbase + o_cd, (const float*)(dbase + o_ca), csr_c, n};
    a.nnratio = nnratio; a.check_ori = check_orientation ? 1 : 0; a.cs = cs;
    a.match = bw.m_out.p; a.nm = a.match + (size_t)ncand * cs;
    a.bin = bw.m_aux.p; a.hist = a.bin + (size_t)ncand * cs;
    CsrArgs ca{};
    ca.side[0] = CsrSide{(const int*)(dbase + o_cn), nullptr, n, csr_c};
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
    int32_t* hout = reinterpret_cast<int32_t*>(c->pin);
    HIP_TRY(c, hipMemcpyAsync(hout, a.match, nout * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    for (int j = 0; j < ncand && n; j++) memcpy(match_out + (size_t)j * n, hout + (size_t)j * cs, (size_t)n * 4);
    memcpy(nmatches, hout + (size_t)ncand * cs, (size_t)ncand * 4);
    return COEB_OK;
}

}  // extern "C"
