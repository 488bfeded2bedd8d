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
