// extract_plan.h -- the extractor's geometry planner: plain C++17, no HIP call (tests/san/san_plan.cpp compiles it with g++ alone).
//
// From the cameras' parameters and the sizes of their resident images, plan_geometry lays out everything the kernels index by:
//   levels and cells    LevelInfo per (camera, level), the cell map of k_fast_cells, the slot / candidate / selection bases
//   resize tables       OpenCV's fixed-point bilinear taps per destination column and row (k_resize and both tile kernels)
//   one-launch spans    what each tile of k_pyramid_tiled owns and needs on every level, and the LDS that takes
//   large-rig plan      the same for the two launches of k_pyramid_tiled4 (TilePlan), by groups of four columns
//   form and slots      which of the three pyramid forms this geometry takes; the slotted output list of the device quadtree
// A mistake here is an out-of-range LDS or global read on the device; extractor.hip only reserves and uploads what this returns.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/orbx.h"

namespace {

constexpr int EDGE_THRESHOLD = 19;   // reference src/ORBextractor.cc:74
constexpr int MIN_BORDER = 16;       // EDGE_THRESHOLD - 3, :772
constexpr int PATCH_SIZE = 31;       // :72
constexpr int HALF_PATCH = 15;       // :73
constexpr int CELL_MAX = 64;         // largest wCell/hCell this build stages in LDS
constexpr int TILE_PITCH = 76;       // LDS pitch of the image tile (CELL_MAX + 6, plus up to 3 bytes of dword alignment, rounded up to 4)
constexpr int SCORE_PITCH = 68;      // LDS pitch of the score map (CELL_MAX + 2 rounded up)
constexpr int MAX_LEVELS = 16;
constexpr int COEF_BITS = 11;        // OpenCV INTER_RESIZE_COEF_BITS

struct LevelInfo {
    int w, h, stride;        // level size, row pitch in bytes (multiple of 64)
    int pyr_off;             // byte offset inside the camera's pyramid buffer
    int n_cols, n_rows, w_cell, h_cell;  // reference :782-788
    int cell_base;           // first global cell id
    int slot_base, slot_cap; // per-cell candidate slots: slot_base + local_cell*slot_cap (u32 units)
    int cand_base;           // dense candidate list of this level (u32 units, in the pinned host buffer)
    int xtab_off, ytab_off;  // resize coefficient tables (valid for level >= 1)
    int xgrp_off;            // the x table once more per group of four destination columns (k_pyramid_tiled4), in groups
    int ini_th, min_th;
    float scale;             // mvScaleFactor[level]
    float patch_size;        // (float)(int)(31 * scale)
    int quota;               // mnFeaturesPerLevel[level]
    int sel_base;            // first slot of this (camera, level) in the device quadtree's output list (quota + 4 slots)
};

// limits of the two tile forms of the pyramid that the planner checks and the kernels are built around
constexpr int PYR_HALO = 16;   // what a tile needs of level 0 beyond its own T x T pixels (13 for 8 levels at 1.2; checked by the host)
constexpr int PYR_MAX_LEVELS = 12;
constexpr int T4_MAX_DW = 16;   // dwords of the base block a thread holds while the tables are on their way: (tw + halo) / 4 x (th + halo) <= 16 x threads (host)

// int2 / int4 of the device tables as plain structs of the same layout (the uploads in extractor.hip assert the sizes)
struct plan_int2 { int x, y; };
struct plan_int4 { int x, y, z, w; };

inline int cv_round(double v) { return (int)std::nearbyint(v); }
inline int cv_floor(double v) { int i = (int)v; return i - (i > v); }
inline int cv_ceil(double v) { int i = (int)v; return i + (i < v); }
inline int align_up(int v, int a) { return (v + a - 1) / a * a; }

struct CamTables {
    orbx_params p;
    std::vector<float> scale, inv_scale, sigma2, inv_sigma2;
    std::vector<int> quota;
};

void build_cam_tables(const orbx_params& p, CamTables& T) {
    T.p = p;
    const int n = p.nlevels;
    const double sf = (double)p.scale_factor;  // the reference stores scaleFactor in a double member
    T.scale.assign(n, 1.0f); T.sigma2.assign(n, 1.0f); T.inv_scale.assign(n, 1.0f); T.inv_sigma2.assign(n, 1.0f);
    for (int i = 1; i < n; ++i) {
        T.scale[i] = (float)((double)T.scale[i - 1] * sf);
        T.sigma2[i] = T.scale[i] * T.scale[i];
    }
    for (int i = 0; i < n; ++i) { T.inv_scale[i] = 1.0f / T.scale[i]; T.inv_sigma2[i] = 1.0f / T.sigma2[i]; }
    T.quota.assign(n, 0);
    const float factor = (float)(1.0 / sf);
    float desired = (float)p.nfeatures * (1 - factor) / (1 - (float)std::pow((double)factor, (double)n));
    int sum = 0;
    for (int l = 0; l < n - 1; ++l) {
        T.quota[l] = cv_round(desired);
        sum += T.quota[l];
        desired *= factor;
    }
    T.quota[n - 1] = std::max(p.nfeatures - sum, 0);
}

void compute_umax(int* umax) {
    int v, v0, vmax = cv_floor(HALF_PATCH * std::sqrt(2.f) / 2 + 1);
    int vmin = cv_ceil(HALF_PATCH * std::sqrt(2.f) / 2);
    const double hp2 = HALF_PATCH * HALF_PATCH;
    for (v = 0; v <= vmax; ++v) umax[v] = cv_round(std::sqrt(hp2 - v * v));
    for (v = HALF_PATCH, v0 = 0; v >= vmin; --v) {
        while (umax[v0] == umax[v0 + 1]) ++v0;
        umax[v] = v0;
        ++v0;
    }
}

// OpenCV resize(INTER_LINEAR) coefficient tables for one axis pair (imgwarp.cpp, 8-bit fixed point path)
void build_resize_tables(int sw, int sh, int dw, int dh, std::vector<plan_int2>& xt, std::vector<plan_int4>& yt) {
    const int ONE = 1 << COEF_BITS;
    const double scale_x = 1. / ((double)dw / sw), scale_y = 1. / ((double)dh / sh);
    auto sat_short = [](int v) { return v < -32768 ? -32768 : v > 32767 ? 32767 : v; };
    for (int dx = 0; dx < dw; ++dx) {
        float fx = (float)((dx + 0.5) * scale_x - 0.5);
        int sx = cv_floor(fx);
        fx -= sx;
        if (sx < 0) { fx = 0; sx = 0; }
        if (sx >= sw - 1) { fx = 0; sx = sw - 1; }
        const int a0 = sat_short(cv_round((1.f - fx) * ONE)), a1 = sat_short(cv_round(fx * ONE));
        const int sx1 = std::min(sx + 1, sw - 1);
        plan_int2 e;
        e.x = (sx & 0xffff) | (sx1 << 16);
        e.y = (a0 & 0xffff) | (a1 << 16);
        xt.push_back(e);
    }
    for (int dy = 0; dy < dh; ++dy) {
        float fy = (float)((dy + 0.5) * scale_y - 0.5);
        int sy = cv_floor(fy);
        fy -= sy;
        plan_int4 e;
        e.x = std::min(std::max(sy, 0), sh - 1);      // each tap's row is clipped, coefficients stay
        e.y = std::min(std::max(sy + 1, 0), sh - 1);
        e.z = sat_short(cv_round((1.f - fy) * ONE));
        e.w = sat_short(cv_round(fy * ONE));
        yt.push_back(e);
    }
}

// k_pyramid_tiled4's view of the x table: per group of four destination columns {c, sel0, sel1, sel2} {sel3, alpha0..2} {alpha3}, c = the
// first tap's source column, sel_j = (left tap - c) | 0x0c << 8 | (right tap - c) << 16 | 0x0c << 24 (v_perm_b32 selector over the
// row's eight bytes from c on: tap | 0 | tap | 0), alpha_j = the column's coefficient pair.  Columns past the level's width repeat
// its last one (they land in the row pitch's padding).
void build_resize_groups(const std::vector<plan_int2>& xt, int xtab_off, int dw, std::vector<plan_int4>& xg) {
    for (int x4 = 0; x4 < dw; x4 += 4) {
        const int c = xt[xtab_off + x4].x & 0xffff;
        uint32_t sel[4], al[4];
        for (int j = 0; j < 4; ++j) {
            const plan_int2 e = xt[xtab_off + std::min(x4 + j, dw - 1)];
            const uint32_t l = (uint32_t)((e.x & 0xffff) - c) & 7u, r = (uint32_t)(((unsigned)e.x >> 16) - c) & 7u;
            sel[j] = l | (0x0cu << 8) | (r << 16) | (0x0cu << 24);
            al[j] = (uint32_t)e.y;
        }
        xg.push_back(plan_int4{c, (int)sel[0], (int)sel[1], (int)sel[2]});
        xg.push_back(plan_int4{(int)sel[3], (int)al[0], (int)al[1], (int)al[2]});
        xg.push_back(plan_int4{(int)al[3], 0, 0, 0});
    }
}

size_t pyramid_bytes(const CamTables& T, int W, int H) {
    size_t off = 0;
    for (int l = 0; l < T.p.nlevels; ++l) {
        const int w = cv_round((double)((float)W * T.inv_scale[l])), h = cv_round((double)((float)H * T.inv_scale[l]));
        off += (size_t)align_up(align_up(w, 64) * h, 256);
    }
    return off;
}

// large rigs: the pyramid as TWO tile launches with four pixels per lane (k_pyramid_tiled4): levels 1..m below level 0 and levels
// m+1.. below level m
struct TilePlan {
    int base = 0, last = 0, tw = 0, th = 0, halo_x = 16, halo_y = 16, tx_max = 0, ty_max = 0, gcap = 0, rcap = 0, lds = 0, threads = 256;
    short tx[64] = {}, ty[64] = {};
    std::vector<plan_int4> sx, sy;   // spans per (camera, level, tile column / row)
    bool ok = false;
};

struct PlanInput {
    const CamTables* cams = nullptr;               // [n_cams]
    const int *cur_w = nullptr, *cur_h = nullptr;  // size of the resident image per camera (0 = none)
    int n_cams = 0, max_levels = 0, max_w = 0, max_h = 0;
    size_t cam_pitch = 0;                          // bytes of pyramid memory per camera
    bool l0_optin = false;                         // orbx_set_inplace_level0
    int t4_plan[3] = {128, 64, 3};                 // tile width / height / split level of the large-rig plan (orbx_debug_pyramid_plan)
    int pyr_chain = -1;                            // MORB_PYR_CHAIN (-1: unset)
};

struct GeometryPlan {
    std::vector<LevelInfo> levels;   // [cam * max_levels + level]
    std::vector<plan_int2> cell_map;
    int cell_h_max = 1, cell_px_max = 1;   // tallest cell / most pixels in a cell over all cameras and levels (k_fast_cells' LDS)
    int total_cells = 0;
    size_t total_slots = 0;
    std::vector<plan_int2> xt;       // resize tables of every level >= 1, LevelInfo::xtab_off / ytab_off / xgrp_off into them
    std::vector<plan_int4> yt, xg;
    // the tiled whole-pyramid launch (k_pyramid_tiled): spans per (camera, level, tile column / row), tiles per camera, LDS need
    std::vector<plan_int4> psx, psy;
    int pyr_tx_max = 0, pyr_ty_max = 0, pyr_lds = 0, pyr_tile = 0, pyr_tab_cap = 0;
    short pyr_tx[64] = {}, pyr_ty[64] = {};
    TilePlan tp[2];
    bool tiled_ok = false;            // this geometry fits the one-launch form (LDS, halo, level count) and is small enough to prefer it
    bool v4_ok = false;               // level steps <= 1.6: the four-pixels-per-lane arithmetic of k_pyramid_tiled4 applies (taps of four neighbours within 8 bytes)
    bool generic_chain = false;       // MORB_PYR_CHAIN=2: neither tile form, one k_resize launch per level
    bool tiled4 = false;              // this geometry takes the two tile launches
    bool l0_on = false;               // level 0 read in place: the geometry takes it (the large-rig tile launches) and the caller opted in
    std::vector<unsigned short> slot_blk;   // slot -> (camera, level) block of the device quadtree's output list
    int total_sel_slots = 0;
};

inline int plan_fail(std::string* why, int rc, const char* fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (why) *why = buf;
    return rc;
}

// ---- level and cell layout, resize tables
int plan_levels(const PlanInput& in, GeometryPlan& G, std::string* why) {
    const int ML = in.max_levels;
    G.levels.assign((size_t)in.n_cams * ML, LevelInfo{});
    int cell_base = 0;
    size_t slot_base = 0, cand_base = 0;
    for (int c = 0; c < in.n_cams; ++c) {
        const CamTables& T = in.cams[c];
        const int W = in.cur_w[c], H = in.cur_h[c];
        if (W == 0 || H == 0) continue;
        int pyr_off = 0, pw = 0, ph = 0;
        for (int l = 0; l < T.p.nlevels; ++l) {
            LevelInfo& Lv = G.levels[(size_t)c * ML + l];
            const float s = T.inv_scale[l];
            Lv.w = cv_round((double)((float)W * s));  // reference :1113-1114
            Lv.h = cv_round((double)((float)H * s));
            Lv.stride = align_up(Lv.w, 64);
            Lv.pyr_off = pyr_off;
            pyr_off += align_up(Lv.stride * Lv.h, 256);
            Lv.ini_th = T.p.ini_th_fast; Lv.min_th = T.p.min_th_fast;
            Lv.scale = T.scale[l];
            Lv.patch_size = (float)(int)(PATCH_SIZE * T.scale[l]);  // :838
            // cell grid, :774-788
            const float width = (float)(Lv.w - 2 * MIN_BORDER), height = (float)(Lv.h - 2 * MIN_BORDER);
            const int nCols = (int)(width / 30.f), nRows = (int)(height / 30.f);
            if (nCols < 1 || nRows < 1)
                return plan_fail(why, ORB_E_ARG, "camera %d level %d is %dx%d: too small for the 30-px detection grid", c, l, Lv.w, Lv.h);
            Lv.n_cols = nCols; Lv.n_rows = nRows;
            Lv.w_cell = (int)std::ceil(width / nCols);
            Lv.h_cell = (int)std::ceil(height / nRows);
            if (Lv.w_cell > CELL_MAX || Lv.h_cell > CELL_MAX || Lv.w > 4096 + 2 * MIN_BORDER || Lv.h > 4096 + 2 * MIN_BORDER)
                return plan_fail(why, ORB_E_ARG, "camera %d level %d (%dx%d): cell %dx%d or level size outside the supported range", c, l,
                                 Lv.w, Lv.h, Lv.w_cell, Lv.h_cell);
            G.cell_h_max = std::max(G.cell_h_max, Lv.h_cell); G.cell_px_max = std::max(G.cell_px_max, Lv.w_cell * Lv.h_cell);
            Lv.quota = T.quota[l];
            Lv.cell_base = cell_base;
            Lv.slot_cap = ((Lv.w_cell + 1) / 2) * ((Lv.h_cell + 1) / 2);  // strict 8-neighbour maxima cannot be denser
            Lv.slot_base = (int)slot_base;
            Lv.cand_base = (int)cand_base;
            const int ncell = nCols * nRows;
            for (int k = 0; k < ncell; ++k)   // {block | cell column << 12 | cell row << 22, local cell index}
                G.cell_map.push_back(plan_int2{(c * ML + l) | ((k % Lv.n_cols) << 12) | ((k / Lv.n_cols) << 22), k});
            cell_base += ncell;
            slot_base += (size_t)ncell * Lv.slot_cap;
            cand_base += (size_t)ncell * Lv.slot_cap;
            if (l > 0) {
                Lv.xtab_off = (int)G.xt.size(); Lv.ytab_off = (int)G.yt.size(); Lv.xgrp_off = (int)(G.xg.size() / 3);
                build_resize_tables(pw, ph, Lv.w, Lv.h, G.xt, G.yt);
                build_resize_groups(G.xt, Lv.xtab_off, Lv.w, G.xg);
            }
            pw = Lv.w; ph = Lv.h;
        }
        if ((size_t)pyr_off > in.cam_pitch) return plan_fail(why, ORB_E_ARG, "image larger than the size given at create");
    }
    G.total_cells = cell_base;
    G.total_slots = slot_base;
    return ORB_OK;
}

// ---- spans of the tiled whole-pyramid launch (k_pyramid_tiled): tile k of a camera owns, on level l, the destination
// columns whose left source tap lies in what it owns on level l - 1 ([k T, (k + 1) T) on level 0), and needs them plus the
// taps of everything it needs one level down; rows alike.  Small rigs take 32-pixel tiles (more workgroups: the launch is
// one round of short workgroups), large ones 64 (less of the halo recomputed).  Also decides between the three pyramid forms
// as far as the large-rig plan's own limits (plan_tile4) do not.
void plan_tile_spans(const PlanInput& in, GeometryPlan& G) {
    const int ML = in.max_levels;
    long long px0 = 0;
    for (int c = 0; c < in.n_cams; ++c) px0 += (long long)in.cur_w[c] * in.cur_h[c];
    const int T = px0 <= 1500000 ? 32 : 64;
    G.pyr_tile = T; G.pyr_tx_max = 1; G.pyr_ty_max = 1; G.pyr_lds = 0; G.pyr_tab_cap = 0;
    bool halo_ok = true;
    for (int c = 0; c < in.n_cams; ++c) {
        G.pyr_tx[c] = (short)((in.cur_w[c] + T - 1) / T); G.pyr_ty[c] = (short)((in.cur_h[c] + T - 1) / T);
        G.pyr_tx_max = std::max<int>(G.pyr_tx_max, G.pyr_tx[c]); G.pyr_ty_max = std::max<int>(G.pyr_ty_max, G.pyr_ty[c]);
    }
    G.psx.assign((size_t)in.n_cams * ML * G.pyr_tx_max, plan_int4{0, 0, 0, 0});
    G.psy.assign((size_t)in.n_cams * ML * G.pyr_ty_max, plan_int4{0, 0, 0, 0});
    // one axis: dims[l], first / last source index of destination d on level l (l >= 1)
    auto axis = [&](int c, int ntiles, int tmax, bool is_x, std::vector<plan_int4>& out) {
        const int NL = in.cams[c].p.nlevels;
        auto dim = [&](int l) { const LevelInfo& Lv = G.levels[(size_t)c * ML + l]; return is_x ? Lv.w : Lv.h; };
        auto s0 = [&](int l, int d) { const LevelInfo& Lv = G.levels[(size_t)c * ML + l]; return is_x ? (G.xt[Lv.xtab_off + d].x & 0xffff) : G.yt[Lv.ytab_off + d].x; };
        auto s1 = [&](int l, int d) { const LevelInfo& Lv = G.levels[(size_t)c * ML + l]; return is_x ? (int)((unsigned)G.xt[Lv.xtab_off + d].x >> 16) : G.yt[Lv.ytab_off + d].y; };
        std::vector<std::vector<int> > b(NL, std::vector<int>(ntiles + 1, 0));
        for (int k = 0; k <= ntiles; ++k) b[0][k] = std::min(k * T, dim(0));
        for (int l = 1; l < NL; ++l) {
            int d = 0;
            for (int k = 0; k <= ntiles; ++k) {   // first destination whose left tap is not in front of the boundary
                while (d < dim(l) && s0(l, d) < b[l - 1][k]) ++d;
                b[l][k] = k == ntiles ? dim(l) : d;
            }
        }
        for (int k = 0; k < ntiles; ++k) {
            int n1 = b[NL - 1][k + 1];
            for (int l = NL - 1; l >= 0; --l) {
                const int nn = n1 - b[l][k];   // .w: 2^20 / needed extent, rounded up (index / extent by multiplication in the kernel)
                out[((size_t)c * ML + l) * tmax + k] = plan_int4{b[l][k], b[l][k + 1], n1, nn > 0 ? (int)(((1u << 20) + nn - 1) / nn) : 0};
                if (l > 0) n1 = std::max(b[l - 1][k + 1], n1 > b[l][k] ? s1(l, n1 - 1) + 1 : b[l - 1][k]);
            }
        }
    };
    for (int c = 0; c < in.n_cams; ++c) {
        if (in.cur_w[c] == 0 || in.cur_h[c] == 0) { G.pyr_tx[c] = G.pyr_ty[c] = 0; continue; }
        axis(c, G.pyr_tx[c], G.pyr_tx_max, true, G.psx);
        axis(c, G.pyr_ty[c], G.pyr_ty_max, false, G.psy);
        for (int ky = 0; ky < G.pyr_ty[c]; ++ky)
            for (int kx = 0; kx < G.pyr_tx[c]; ++kx) {
                int bytes = 0, tx_n = 0, ty_n = 0;
                for (int l = 0; l < in.cams[c].p.nlevels; ++l) {
                    const plan_int4 X = G.psx[((size_t)c * ML + l) * G.pyr_tx_max + kx], Y = G.psy[((size_t)c * ML + l) * G.pyr_ty_max + ky];
                    if (l == 0) {   // the kernel stages a fixed (T + halo)^2 block of level 0: what the tile needs must lie inside it
                        bytes += (T + PYR_HALO) * (T + PYR_HALO);
                        if (X.z - X.x > T + PYR_HALO || Y.z - Y.x > T + PYR_HALO) halo_ok = false;
                        continue;
                    }
                    bytes += ((std::max(X.z - X.x, 0) + 3) & ~3) * std::max(Y.z - Y.x, 0);
                    tx_n += std::max(X.z - X.x, 0); ty_n += std::max(Y.z - Y.x, 0);
                }
                G.pyr_lds = std::max(G.pyr_lds, bytes);
                G.pyr_tab_cap = std::max(G.pyr_tab_cap, std::max(tx_n, ty_n));
            }
    }
    G.pyr_tab_cap = (G.pyr_tab_cap + 3) & ~3;
    G.pyr_lds += G.pyr_tab_cap * 24;   // the table entries of a tile's columns (int2) and rows (int4) in front of the regions
    G.tiled_ok = !(G.pyr_lds > 60 * 1024 || ML > PYR_MAX_LEVELS || !halo_ok || in.max_w > 32767 || in.max_h > 32767);   // (cannot happen for tiles of 64 and scale factors >= 1.05)
    // Large rigs take two tile launches with four pixels per lane instead (k_pyramid_tiled4, plan_tile4): the one-launch tile kernel is a
    // latency design and costs three times the instructions per pixel.  Their arithmetic needs level steps of at most 1.6 (the taps of
    // four neighbouring pixels within 8 bytes).  MORB_PYR_CHAIN: 1 = the large-rig form at every size, 2 = neither tile form (the
    // generic one-launch-per-level chain, k_resize: what odd parameter sets fall back to), 0 = never the large-rig form; default: the
    // large-rig form above 4 M level-0 pixels over all cameras (8 x 1080p yes, 2 x 1280x720 no).
    G.v4_ok = true;
    for (int c = 0; c < in.n_cams && G.v4_ok; ++c)
        for (int l = 1; l < in.cams[c].p.nlevels; ++l) {
            const LevelInfo &Ls = G.levels[(size_t)c * ML + l - 1], &Ld = G.levels[(size_t)c * ML + l];
            if (Ld.w > 0 && (long long)Ls.w * 10 > (long long)Ld.w * 16) G.v4_ok = false;
        }
    G.generic_chain = in.pyr_chain == 2;
    const bool prefer_large = G.v4_ok && (in.pyr_chain == 1 || (in.pyr_chain < 0 && (long long)px0 > 4000000ll));
    if (prefer_large || G.generic_chain) G.tiled_ok = false;
}

// One axis of one camera in a TilePlan.  Along x a tile owns whole groups of four destination columns (the group whose first tap lies
// in what the tile owns one level up) and its boundaries are pixels that are multiples of four below the base; along y it owns rows
// by their upper tap.  Writes the spans of tiles 0 .. nt - 1 on levels P.base .. NL and raises `need` to the widest base-level need.
void plan_tile4_axis(const GeometryPlan& G, const TilePlan& P, int ML, int c, int NL, bool is_x, std::vector<plan_int4>& out, int& need) {
    auto LV = [&](int l) -> const LevelInfo& { return G.levels[(size_t)c * ML + l]; };
    const int nt = is_x ? P.tx[c] : P.ty[c], tile = is_x ? P.tw : P.th, tmax = is_x ? P.tx_max : P.ty_max, U = is_x ? 4 : 1;
    auto dim = [&](int l) { return is_x ? LV(l).w : LV(l).h; };
    auto units = [&](int l) { return (dim(l) + U - 1) / U; };   // groups of four columns, or rows
    auto first_tap = [&](int l, int u) { return is_x ? (G.xt[LV(l).xtab_off + 4 * u].x & 0xffff) : G.yt[LV(l).ytab_off + u].x; };
    // (padding columns of the last group repeat the level's last one)
    auto last_tap = [&](int l, int d) { return is_x ? (int)((unsigned)G.xt[LV(l).xtab_off + std::min(d, LV(l).w - 1)].x >> 16) : G.yt[LV(l).ytab_off + d].y; };
    std::vector<std::vector<int> > b(ML, std::vector<int>(nt + 1, 0));
    for (int k = 0; k <= nt; ++k) b[P.base][k] = std::min(k * tile, dim(P.base));
    for (int l = P.base + 1; l <= NL; ++l) {
        int u = 0;
        for (int k = 0; k <= nt; ++k) {
            while (u < units(l) && first_tap(l, u) < b[l - 1][k]) ++u;
            b[l][k] = U * (k == nt ? units(l) : u);
        }
    }
    for (int k = 0; k < nt; ++k) {
        int n1 = b[NL][k + 1];
        for (int l = NL; l >= P.base; --l) {
            const int ngn = is_x && l > P.base ? std::max(n1 - b[l][k], 0) / 4 : 0;   // x .w: 2^20 / needed groups, rounded up; y .w: 0
            out[((size_t)c * ML + l) * tmax + k] = plan_int4{b[l][k], b[l][k + 1], n1, ngn > 0 ? (int)(((1u << 20) + ngn - 1) / ngn) : 0};
            if (l == P.base) { need = std::max(need, n1 - b[l][k]); break; }
            // what level l - 1 must hold: its own run, and the right / lower tap of the last column / row this level needs
            int up = b[l - 1][k + 1];
            if (n1 > b[l][k]) up = std::max(up, last_tap(l, n1 - 1) + 1);
            n1 = is_x && l - 1 > P.base ? std::min((up + 3) & ~3, 4 * units(l - 1)) : up;
        }
    }
}

// ---- large rigs: the two tile launches of k_pyramid_tiled4 (TilePlan).  What a tile needs beyond what it owns is the taps of
// everything it needs one level down (rounded up to whole groups below the base).
void plan_tile4(const PlanInput& in, GeometryPlan& G) {
    const int ML = in.max_levels;
    G.tiled4 = false;
    // tile 128 x 64 below level 0 and below the split level 3, 256 threads (orbx_debug_pyramid_plan: other tiles / another split, for
    // the tests of the plan's geometry)
    const int split_env = in.t4_plan[2], tw_env = in.t4_plan[0], th_env = in.t4_plan[1];
    int nl_max = 0;
    for (int c = 0; c < in.n_cams; ++c) nl_max = std::max(nl_max, in.cams[c].p.nlevels);
    const bool want = G.v4_ok && !G.tiled_ok && !G.generic_chain && nl_max >= 2 && ML <= PYR_MAX_LEVELS &&
                      tw_env >= 16 && tw_env % 4 == 0 && th_env >= 8 && in.max_w <= 32767 && in.max_h <= 32767;
    const int split = std::min(std::max(split_env, 1), nl_max - 1);
    bool all_ok = want;
    for (int pi = 0; pi < 2 && all_ok; ++pi) {
        TilePlan& P = G.tp[pi];
        P.ok = false;
        P.base = pi == 0 ? 0 : split; P.last = pi == 0 ? split : nl_max - 1;
        if (P.last <= P.base) { P.ok = true; P.tx_max = P.ty_max = 0; continue; }   // (nothing left for the second launch)
        P.tw = tw_env; P.th = th_env; P.halo_x = 16; P.halo_y = 16;
        P.threads = 256;
        P.tx_max = P.ty_max = 1; P.gcap = P.rcap = 0; P.lds = 0;
        for (int c = 0; c < in.n_cams; ++c) {
            const LevelInfo& Lb = G.levels[(size_t)c * ML + P.base];
            P.tx[c] = (short)(Lb.w > 0 ? (Lb.w + P.tw - 1) / P.tw : 0); P.ty[c] = (short)(Lb.w > 0 ? (Lb.h + P.th - 1) / P.th : 0);
            P.tx_max = std::max<int>(P.tx_max, P.tx[c]); P.ty_max = std::max<int>(P.ty_max, P.ty[c]);
        }
        P.sx.assign((size_t)in.n_cams * ML * P.tx_max, plan_int4{0, 0, 0, 0});
        P.sy.assign((size_t)in.n_cams * ML * P.ty_max, plan_int4{0, 0, 0, 0});
        bool ok = true;
        int need_x = P.tw, need_y = P.th;   // what a tile needs of the base level, at most (the staged block: tile + halo)
        for (int c = 0; c < in.n_cams; ++c) {
            if (P.tx[c] == 0) continue;
            const int NL = std::min(in.cams[c].p.nlevels - 1, P.last);   // last level this camera has inside the plan
            plan_tile4_axis(G, P, ML, c, NL, true, P.sx, need_x);
            plan_tile4_axis(G, P, ML, c, NL, false, P.sy, need_y);
        }
        P.halo_x = ((need_x - P.tw + 3) & ~3); P.halo_y = need_y - P.th;
        // what a workgroup holds in LDS: the staged base block, the regions of its levels, the table entries of their groups and rows
        for (int c = 0; c < in.n_cams && ok; ++c) {
            if (P.tx[c] == 0) continue;
            const int NL = std::min(in.cams[c].p.nlevels - 1, P.last);
            for (int ky = 0; ky < P.ty[c]; ++ky)
                for (int kx = 0; kx < P.tx[c]; ++kx) {
                    int bytes = (P.tw + P.halo_x) * (P.th + P.halo_y), ng = 0, nr = 0;
                    for (int l = P.base + 1; l <= NL; ++l) {
                        const plan_int4 X = P.sx[((size_t)c * ML + l) * P.tx_max + kx], Y = P.sy[((size_t)c * ML + l) * P.ty_max + ky];
                        const int w = std::max(X.z - X.x, 0), h = std::max(Y.z - Y.x, 0);
                        if ((long long)(w / 4) * h * (w / 4) >= (1 << 20)) ok = false;   // (index split by multiplication: tasks x groups < 2^20)
                        bytes += w * h; ng += w / 4; nr += h;
                    }
                    P.lds = std::max(P.lds, bytes); P.gcap = std::max(P.gcap, ng); P.rcap = std::max(P.rcap, nr);
                }
        }
        P.gcap = std::max(P.gcap, 1); P.rcap = std::max(P.rcap, 1);
        P.lds += P.gcap * 48 + P.rcap * 16 + 32;
        if (P.lds > 64 * 1024 || (P.tw + P.halo_x) / 4 * (P.th + P.halo_y) > T4_MAX_DW * P.threads || (P.halo_x & 3)) ok = false;
        P.ok = ok;
        all_ok = all_ok && ok;
    }
    G.tiled4 = all_ok;
}

// ---- slotted output list of the device quadtree: quota + 4 slots per (camera, level)
void plan_slot_blocks(GeometryPlan& G) {
    for (size_t b = 0; b < G.levels.size(); ++b) {
        LevelInfo& Lv = G.levels[b];
        Lv.sel_base = (int)G.slot_blk.size();
        if (Lv.w == 0) continue;
        for (int k = 0; k < Lv.quota + 4; ++k) G.slot_blk.push_back((unsigned short)b);
    }
    G.total_sel_slots = (int)G.slot_blk.size();
}

// Everything above in order; `G` is rebuilt from nothing.  ORB_OK, or ORB_E_ARG with the reason in `why`.
int plan_geometry(const PlanInput& in, GeometryPlan& G, std::string* why) {
    G = GeometryPlan{};
    if (int rc = plan_levels(in, G, why)) return rc;
    plan_tile_spans(in, G);
    plan_tile4(in, G);
    // level 0 is read where the caller's device image lies (orbx_set_inplace_level0) by the large-rig tile launches only: they take
    // the {pointer, pitch} table; the one-launch tile kernel of small rigs and the generic chain read the pyramid buffer
    G.l0_on = in.l0_optin && G.tiled4;
    if (G.total_slots > (size_t)INT32_MAX) return plan_fail(why, ORB_E_ARG, "candidate slot space exceeds 2^31 entries");
    plan_slot_blocks(G);
    return ORB_OK;
}

}  // namespace
