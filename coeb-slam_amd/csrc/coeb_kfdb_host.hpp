// coeb_kfdb_host.hpp -- the host half of the keyframe database (coeb_kfdb.hip): the arithmetic of
// KeyFrameDatabase::DetectRelocalizationCandidates (src/KeyFrameDatabase.cc:199-253) that needs no
// device, kept apart so that it is tested without one.  Host code only (no HIP).
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/coeb_front.h"

// int minCommonWords = maxCommonWords * 0.8f  (:235): a float multiply, truncated
int kfdb_min_common(int max_common);

// lKFsSharingWords (:207-222): the slots with common > 0 in the order the inverted file meets them
// first -- ascending smallest common word, then insertion sequence.  first_word[slot] is read only
// where common[slot] > 0.  order holds nslots entries; returns the list's length.
int kfdb_sharing_order(const int32_t* common, const int32_t* first_word, const int64_t* seq, int nslots, int32_t* order);

// bow_word strictly ascending and non-negative
bool kfdb_words_ascending(const int32_t* word, int nw);

// ---- LocalMapping::CreateNewMapPoints' SearchForTriangulation over stored keyframes ----
// What coeb_kfdb_set_geometry keeps of one feature: mvKeysUn[i].pt, mvuRight[i], mvKeysUn[i].octave.
struct KfdbGeo { float x, y, u_right; int32_t octave; };
static_assert(sizeof(KfdbGeo) == 16, "the geometry slab holds 16 bytes per feature");

// out[0 .. n) from the keyframe's arrays; false, with out unspecified, when an octave lies outside 0 .. nlevels - 1
bool kfdb_pack_geometry(const coeb_keypoint* keys_un, const float* u_right, int n, int nlevels, KfdbGeo* out);

// The rules of coeb_kfdb_search_triangulation's arguments that need no device.  used / geo / n describe
// the slots [0, nslots).  nullptr: the call may go on; else the text of its COEB_EINVAL.
const char* kfdb_tri_check(const uint8_t* used, const uint8_t* geo, const int* n, int nslots, int slot1,
                           const uint8_t* has_mp1, const int32_t* slots2, int nnb, const uint8_t* const* has_mp2,
                           const float* F12, const float* epipole, const int32_t* match_out, const int32_t* nmatches);

// The neighbours' masks one after the other at 16-byte rounded offsets of `masks`, and the table the
// kernel reads: tab[2 j] = slots2[j], tab[2 j + 1] = the offset of has_mp2[j] in masks.
void kfdb_tri_pack(const int* n, const int32_t* slots2, int nnb, const uint8_t* const* has_mp2,
                   std::vector<uint8_t>& masks, std::vector<int32_t>& tab);

// ---- LocalMapping::SearchInNeighbors' Fuse search over stored keyframes ----
// One job as k_fuse reads it: the slot, the range of the list, where its results start, where its skip
// bytes start in the packed skip array (-1: none), and the keyframe's pose.
struct KfdbFuseJob { int32_t slot, first, count, out_off, skip_off; float Rcw[9], tcw[3], Ow[3]; };
static_assert(sizeof(KfdbFuseJob) == 80, "the job table holds 80 bytes per job");

// The bounds a slot's feature grid was built with (coeb_kfdb_fuse_search); built == 0: no grid.
struct KfdbGridRec { uint8_t built; float min_x, max_x, min_y, max_y; };
bool kfdb_grid_current(const KfdbGridRec& r, const coeb_camera* cam);

// The rules of coeb_kfdb_fuse_search's arguments that need no device.  nullptr: the call may go on, with
// *total = the sum of the counts; else the text of its error and *code = COEB_EINVAL or COEB_ERANGE.
const char* kfdb_fuse_check(const uint8_t* used, const uint8_t* geo, int nslots, const coeb_camera* cam,
                            const coeb_fuse_points* pts, const coeb_fuse_job* jobs, int njobs, float th,
                            const int32_t* best_idx, const int32_t* best_dist, int* code, int64_t* total);

// The job table, the skip bytes of all jobs one after the other at 16-byte rounded offsets, and the
// distinct slots whose grid has to be built (rec[slot] not current for cam), ascending.
void kfdb_fuse_pack(const coeb_fuse_job* jobs, int njobs, const KfdbGridRec* rec, const coeb_camera* cam,
                    std::vector<KfdbFuseJob>& tab, std::vector<uint8_t>& skip, std::vector<int32_t>& build);

// ---- the rest of LocalMapping::CreateNewMapPoints' loop body over stored keyframes ----
// What coeb_kfdb_set_stereo keeps of one feature: the raw mvKeys[i].pt and mvDepth[i] that
// KeyFrame::UnprojectStereo and the parallax bound read.
struct KfdbStereo { float kx, ky, depth, pad; };
static_assert(sizeof(KfdbStereo) == 16, "the stereo slab holds 16 bytes per feature");

// out[0 .. n) from the keyframe's arrays (key_xy [n][2]), depth_pos[i] = depth[i] > 0; false, with out
// unspecified, when an entry is not finite
bool kfdb_pack_stereo(const float* key_xy, const float* depth, int n, KfdbStereo* out, uint8_t* depth_pos);

// a feature with u_right >= 0 whose depth is not positive: UnprojectStereo would return an empty Mat
bool kfdb_stereo_conflict(const uint8_t* is_stereo, const uint8_t* depth_pos, int n);

// What k_tri_points writes per (neighbour, feature of keyframe 1): the way out of the loop body in the low
// four bits, the source of x3D (COEB_NEWPTS_SRC_*) in bits 4 and 5.
enum {
    kNpNoPair = 0, kNpAccepted = 1, kNpLowParallax = 2, kNpW0 = 3, kNpZ1 = 4, kNpZ2 = 5, kNpReproj1 = 6,
    kNpReproj2 = 7, kNpZeroDist = 8, kNpRatio = 9,
};

// The rules of coeb_kfdb_create_new_map_points' arguments that need no device, behind those of
// kfdb_tri_check.  stereo[slot] != 0: the slot has its stereo data; conflict[slot] != 0:
// kfdb_stereo_conflict holds for it.  nullptr: the call may go on; else the text of its COEB_EINVAL.
const char* kfdb_newpts_check(const uint8_t* used, const uint8_t* geo, const uint8_t* stereo, const uint8_t* conflict,
                              const int* n, int nslots, int slot1, const coeb_kf_view* view1, const uint8_t* has_mp1,
                              const int32_t* slots2, int nnb, const coeb_kf_view* views2, const uint8_t* const* has_mp2,
                              const float* F12, const float* epipole, const int32_t* match_out, const int8_t* status,
                              const float* x3d, const int32_t* first_ok, const int32_t* nmatches);

// What the host does with the downloaded rows: x3d of the accepted entries into the caller's array (every other
// entry untouched), first_ok's INT_MAX to -1, nmatches[j] = the pairs of row j.
void kfdb_newpts_unpack(const int32_t* match, const int8_t* status, const float* x3d_dev, const int32_t* first_dev,
                        int nnb, int n1, float* x3d, int32_t* first_ok, int32_t* nmatches);
