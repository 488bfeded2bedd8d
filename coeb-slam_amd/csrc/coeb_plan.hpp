// coeb_plan.hpp -- the extraction's geometry plan: the ORBextractor tables of a context and, per
// image size, every buffer offset, resize-table index, FAST cell and LDS size the extraction
// kernels use (built by coeb_plan.cpp).  Plain C++ with no HIP type, so
// tests/host/plan_host_main.cpp runs the builder under ASan + UBSan without a device.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/coeb_front.h"

#define COEB_MAXL 16
#define COEB_MAXBOX 16

// Per-level geometry and offsets, computed on the host once per (W, H) and copied to the
// device as one POD block (kernel argument).
struct LevelGeom {
    int w, h;
    int pitch;             // row pitch of the level image (level 0: W; levels >= 1: 64-byte multiple)
    int bpitch;            // row pitch of the blurred level (64-byte multiple)
    int64_t pyr_off;       // into pyr frame block (-1 for level 0)
    int64_t blur_off;      // into blur frame block
    int rtab_off;          // into resize table (ints): xofs[w], alpha[w], yofs[h], beta[h]
    int xmax;              // resize: columns >= xmax use S[sx]*2048
    int rows_ok;           // k_pyr_rows applies: every even column pair's sources within 6 bytes of
                           // the pair's 4-byte aligned window start (scale <= 2)
    int yrow_off;          // into resize table (ints): per output row {r0 * sp, r1 * sp, beta, dy * pitch}
                           // (the clamped source rows' byte offsets; sp = the source level's pitch)
    int band_off;          // into resize table (ints): per 8-row output band one PyrBand descriptor
    int ncols, nrows, wcell, hcell;
    int cell0, ncells;     // range in the cell table (row-major over non-skipped cells)
    int kcap_off, kcap;    // octree key buffers: offset / capacity (u32 entries)
    int nfeat, nfeat_area; // DistributeOctTree N: mnFeaturesPerLevel[l], (int)(N*0.7)
    int nini;              // initial octree nodes
    float hx;              // (maxX-minX)/nIni
    int ini_bound[5];      // initial node i holds x_rel in [ini_bound[i], ini_bound[i+1])
    int ncap;              // node record capacity per set
    int64_t node_off;      // into node scratch (records) per frame
    int out_cap, out_off;  // level keypoint capacity / offset into lvl_kp frame block
    float scale;           // mvScaleFactor[l]
    int size_i;            // (int)(PATCH_SIZE * scale)
    int maxX, maxY;        // octree box: maxBorderX - minBorderX, maxBorderY - minBorderY
};

// k_pyr_rows' band descriptors.  A band is 8 consecutive output rows oy .. oy + 7 (one wave's
// rows); its row pattern is the sequence sy(oy + r) - sy(oy), r = 0..7, of the rows' first source
// rows, written as a 7-bit mask: bit i set where sy(oy + i + 1) - sy(oy + i) is 2 (else it is 1).
// A band with mask m reads the 9 + popcount(m) consecutive source rows sy(oy) .. sy(oy + 7) + 1.
// At the cascade's scale of ~1.2 a double step comes every 5 output rows, which leaves the five
// masks below, one per phase; the real ratios (640/533, ...) drift through them down the image
// and, where the drift crosses a phase, give another mask in one band (1-2 % of the bands of
// 640x480 and 1280x960, from whose plans this list is taken).  Such a band is generic, like a
// band with a clamped source row and a level's last, partial band: the kernel's per-row body.
constexpr int kPyrBandRows = 8;
constexpr int kPyrPatterns = 5;
constexpr unsigned kPyrPatternMask[kPyrPatterns] = {0x10, 0x08, 0x04, 0x42, 0x21};
constexpr int kPyrBandGeneric = -1;
constexpr int kPyrBandInts = 12;
struct PyrBand {           // kPyrBandInts ints in the resize table, 16-byte aligned
    int pattern;           // index into kPyrPatternMask, or kPyrBandGeneric
    int src_off;           // byte offset of the band's first source row: clamp(sy(oy)) * sp
    int dst_off;           // byte offset of the band's first output row: oy * pitch
    int pad;
    int beta[kPyrBandRows];   // the rows' beta entries (0 past the level's last row)
};

struct Plan {
    int W, H, L;
    LevelGeom lv[COEB_MAXL];
    int ncells;            // all levels
    int cell_cap;          // u32 entries per cell slot
    int max_roi_w, max_roi_h;
    int64_t pyr_stride, blur_stride;
    int64_t kbuf_stride;   // u32 entries per key buffer (x2 per frame)
    int64_t node_stride;   // node records per frame (all levels, both sets)
    int lvl_stride;        // u32 entries per frame in lvl_kp
    int kcap;              // output keypoints per frame (sum of out_cap)
    int rtab_ints;
    int umax[16];
    int gauss[7];
    int oct_w;             // k_octree: node records per set / work-list entries (max ncap)
    int oct_kl;            // k_octree: keys kept in LDS when a level has <= oct_kl candidates
    int oct_lds;           // k_octree dynamic LDS bytes
};

// FAST cell descriptor (ORBextractor.cc:811-829): ROI in level coordinates
struct CellDesc {
    int16_t level, pad;
    int16_t x0, y0;        // iniX, iniY
    int16_t rw, rh;        // maxX-iniX, maxY-iniY (ROI; detection window = inset 3)
    int16_t i, j;          // cell row / column (for x_rel/y_rel offsets)
};

struct Tables {
    int nfeatures;
    double scale_factor;   // ORBextractor.h:114 `double scaleFactor`
    int nlevels;
    float scale[COEB_MAXL], inv_scale[COEB_MAXL], sigma2[COEB_MAXL], inv_sigma2[COEB_MAXL];
    int nfeat[COEB_MAXL];
    int umax[16];
};

// ORBextractor::ORBextractor (src/ORBextractor.cc:418-477); false: parameters out of range
bool make_tables(const coeb_orb_params& prm, Tables& t);
// Gaussian 7-tap sigma 2, Q8 error-diffused
void gauss_kernel7(int k[7]);
// cv::resize INTER_LINEAR coefficient tables (imgproc resize.cpp, 8U fixed point) appended to
// tab as xofs[dw], alpha[dw], yofs[dh], beta[dh]; returns xmax
int resize_tables(int sw, int sh, int dw, int dh, std::vector<int>& tab);
// The PyrBand pattern of the output rows oy .. oy + 7 of a level of dh rows resized from sh rows
// (yofs: resize_tables' unclamped first source rows): an index into kPyrPatternMask, or
// kPyrBandGeneric.
int pyr_band_pattern(const int* yofs, int oy, int dh, int sh);
// The plan of a W x H image with its resize tables / row descriptors (rtab) and FAST cells;
// false with err set when the size is not supported.  oct_kl_override: 0, or the keys k_octree
// keeps in LDS per level (clamped to [256, 8192]) in place of the computed count.
bool make_plan(const Tables& t, int W, int H, int oct_kl_override, Plan& P, std::vector<int>& rtab,
               std::vector<CellDesc>& cells, std::string& err);
// k_octree's key capacity of one launch over F frames: *kl keys per level in LDS (more
// candidates: the global ping-pong buffers) and *lds dynamic LDS bytes.  Small batches (per-rank
// shards: fewer workgroups than two per CU, F * L <= 512) double the plan's capacity up to 4096
// keys within 150 KB, so a 1280x960 level 0 (~2 700 candidates) keeps its keys in LDS; large
// batches keep the plan's capacity, which leaves more workgroups per CU.
void oct_launch_keys(const Plan& plan, int F, int* kl, int* lds);
