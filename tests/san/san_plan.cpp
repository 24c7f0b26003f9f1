// ASan + UBSan driver over the extractor's geometry planner (multi_orb_slam_amd/csrc/extract_plan.h; plain C++, nothing of HIP).
// It plans a list of rigs and checks what the kernels rely on: every assertion restates an index a kernel forms from the plan.
// Citations: "x:N" = multi_orb_slam_amd/csrc/extractor.hip line N.
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "../../multi_orb_slam_amd/csrc/extract_plan.h"

static int bad = 0;
static std::string g_rig;
#define CHECK(cond, ...) do { if (!(cond)) { if (++bad <= 30) { std::printf("FAIL [%s] %s:%d %s -- ", g_rig.c_str(), __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static orbx_params params(int nlevels = 8, float sf = 1.2f, int nfeatures = 1000) {
    orbx_params p;
    std::memset(&p, 0, sizeof p);
    p.nfeatures = nfeatures; p.scale_factor = sf; p.nlevels = nlevels; p.ini_th_fast = 20; p.min_th_fast = 7;
    return p;
}

struct Rig {
    std::string name;
    std::vector<orbx_params> p;
    std::vector<int> w, h;          // resident image per camera (0 x 0: an empty camera)
    int chain = -1;                 // MORB_PYR_CHAIN
    int t4[3] = {128, 64, 3};       // orbx_debug_pyramid_plan
    bool l0 = false;
    int max_w = 0, max_h = 0;       // the size given at create (0: the largest image of the rig)
};

static Rig rig(const std::string& name, int n, int w, int h, const orbx_params& p = params(), int chain = -1) {
    Rig r;
    r.name = name; r.p.assign(n, p); r.w.assign(n, w); r.h.assign(n, h); r.chain = chain;
    return r;
}

struct Planned {
    std::vector<CamTables> cams;
    PlanInput in;
    GeometryPlan G;
    std::string why;
    int rc = 0;
};

// what orbx_create and rebuild_geometry hand to the planner
static void plan(const Rig& r, Planned& P) {
    const int n = (int)r.p.size();
    P.cams.resize(n);
    PlanInput& in = P.in;
    in = PlanInput{};
    in.n_cams = n; in.max_w = r.max_w; in.max_h = r.max_h;
    for (int c = 0; c < n; ++c) { in.max_w = std::max(in.max_w, r.w[c]); in.max_h = std::max(in.max_h, r.h[c]); }
    for (int c = 0; c < n; ++c) {
        build_cam_tables(r.p[c], P.cams[c]);
        in.max_levels = std::max(in.max_levels, r.p[c].nlevels);
        in.cam_pitch = std::max(in.cam_pitch, pyramid_bytes(P.cams[c], in.max_w, in.max_h));
    }
    in.cam_pitch = (in.cam_pitch + 4095) / 4096 * 4096 + 4096;
    in.cams = P.cams.data(); in.cur_w = r.w.data(); in.cur_h = r.h.data();
    in.l0_optin = r.l0; in.pyr_chain = r.chain;
    for (int i = 0; i < 3; ++i) in.t4_plan[i] = r.t4[i];
    P.why.clear();
    P.rc = plan_geometry(in, P.G, &P.why);
}

static uint32_t umul24(uint32_t a, uint32_t b) { return (uint32_t)((uint64_t)(a & 0xffffffu) * (uint64_t)(b & 0xffffffu)); }
static int x_tap0(const GeometryPlan& G, const LevelInfo& Lv, int d) { return G.xt[Lv.xtab_off + d].x & 0xffff; }
static int x_tap1(const GeometryPlan& G, const LevelInfo& Lv, int d) { return (int)((unsigned)G.xt[Lv.xtab_off + d].x >> 16); }

// 1. level layout
static void check_levels(const Planned& P) {
    const PlanInput& in = P.in; const GeometryPlan& G = P.G; const int ML = in.max_levels;
    CHECK((int)G.levels.size() == in.n_cams * ML, "levels");
    int cell = 0; long long slot = 0; int sel = 0;
    for (int c = 0; c < in.n_cams; ++c)
        for (int l = 0; l < ML; ++l) {
            const LevelInfo& Lv = G.levels[(size_t)c * ML + l];
            const bool live = in.cur_w[c] > 0 && in.cur_h[c] > 0 && l < in.cams[c].p.nlevels;
            CHECK(Lv.sel_base == sel, "cam %d level %d sel_base %d, running sum %d", c, l, Lv.sel_base, sel);   // k_describe: slot -> block via slot_blk
            CHECK((Lv.w > 0) == live, "cam %d level %d w %d", c, l, Lv.w);
            if (!live) continue;
            // every kernel addresses a level as pyr + cam * cam_pitch + pyr_off + y * stride + x (x:160-161, whole dwords up to the pitch: x:179)
            CHECK(Lv.stride >= Lv.w && Lv.stride % 64 == 0 && Lv.pyr_off % 256 == 0, "cam %d level %d stride %d off %d", c, l, Lv.stride, Lv.pyr_off);
            CHECK((size_t)Lv.pyr_off + (size_t)Lv.stride * Lv.h <= in.cam_pitch, "cam %d level %d ends at %zu, pitch %zu", c, l, (size_t)Lv.pyr_off + (size_t)Lv.stride * Lv.h, in.cam_pitch);
            if (l > 0) { const LevelInfo& Lp = G.levels[(size_t)c * ML + l - 1]; CHECK(Lv.pyr_off >= Lp.pyr_off + Lp.stride * Lp.h, "cam %d level %d overlaps the level above", c, l); }
            else CHECK(Lv.pyr_off == 0 && Lv.w == in.cur_w[c] && Lv.h == in.cur_h[c], "cam %d level 0", c);   // level 0 at offset 0 (orbx_upload, x:248-249)
            CHECK(Lv.cell_base == cell && Lv.slot_base == slot && Lv.cand_base == slot, "cam %d level %d bases %d %d %d, sums %d %lld", c, l, Lv.cell_base, Lv.slot_base, Lv.cand_base, cell, slot);
            CHECK(Lv.n_cols >= 1 && Lv.n_rows >= 1 && Lv.w_cell <= CELL_MAX && Lv.h_cell <= CELL_MAX, "cam %d level %d cells", c, l);
            // the cells cover the detection area (reference :782-788) and fit k_fast_cells' LDS tile
            CHECK(Lv.n_cols * Lv.w_cell >= Lv.w - 2 * MIN_BORDER && Lv.n_rows * Lv.h_cell >= Lv.h - 2 * MIN_BORDER, "cam %d level %d grid", c, l);
            CHECK(Lv.h_cell <= G.cell_h_max && Lv.w_cell * Lv.h_cell <= G.cell_px_max, "cam %d level %d cell maxima", c, l);
            for (int k = 0; k < Lv.quota + 4; ++k)
                if (!(sel + k < (int)G.slot_blk.size() && G.slot_blk[sel + k] == c * ML + l)) { CHECK(false, "cam %d level %d slot_blk[%d]", c, l, sel + k); break; }
            cell += Lv.n_cols * Lv.n_rows; slot += (long long)Lv.n_cols * Lv.n_rows * Lv.slot_cap; sel += Lv.quota + 4;
        }
    CHECK(G.total_cells == cell && (long long)G.total_slots == slot && G.total_sel_slots == sel && (int)G.slot_blk.size() == sel, "totals");
    CHECK((int)G.cell_map.size() == G.total_cells, "cell_map has %zu entries, %d cells", G.cell_map.size(), G.total_cells);
    for (int i = 0; i < (int)G.cell_map.size(); ++i) {   // the decode of k_fast_cells (x:756-757); the cell's slots: x:889
        const plan_int2 cm = G.cell_map[i];
        const int blk = cm.x & 0xfff, cj = (cm.x >> 12) & 0x3ff, ci = (int)((unsigned)cm.x >> 22);
        if (!(blk < (int)G.levels.size())) { CHECK(false, "cell %d block %d", i, blk); break; }
        const LevelInfo& Lv = G.levels[blk];
        if (!(Lv.w > 0 && cj < Lv.n_cols && ci < Lv.n_rows && cm.y == ci * Lv.n_cols + cj && i == Lv.cell_base + cm.y)) { CHECK(false, "cell %d decodes to block %d column %d row %d local %d", i, blk, cj, ci, cm.y); break; }
    }
}

// 2. resize tables: k_resize reads s0[sx0], s0[sx1] of rows yt.x, yt.y of level l - 1 (x:162-174); the tile kernels read the same entries
static void check_tables(const Planned& P) {
    const PlanInput& in = P.in; const GeometryPlan& G = P.G; const int ML = in.max_levels;
    for (int c = 0; c < in.n_cams; ++c)
        for (int l = 1; l < ML; ++l) {
            const LevelInfo &D = G.levels[(size_t)c * ML + l], &S = G.levels[(size_t)c * ML + l - 1];
            if (D.w == 0) continue;
            CHECK(D.xtab_off >= 0 && D.xtab_off + D.w <= (int)G.xt.size() && D.ytab_off >= 0 && D.ytab_off + D.h <= (int)G.yt.size(), "cam %d level %d table range", c, l);
            CHECK(3 * (D.xgrp_off + (D.w + 3) / 4) <= (int)G.xg.size(), "cam %d level %d group range", c, l);
            for (int x = 0; x < D.w; ++x) {
                const int a = x_tap0(G, D, x), b = x_tap1(G, D, x);
                if (!(a >= 0 && a <= b && b < S.w && b <= a + 1)) { CHECK(false, "cam %d level %d column %d taps %d %d of %d", c, l, x, a, b, S.w); break; }
            }
            for (int y = 0; y < D.h; ++y) {
                const plan_int4 e = G.yt[D.ytab_off + y];
                if (!(e.x >= 0 && e.x <= e.y && e.y < S.h)) { CHECK(false, "cam %d level %d row %d taps %d %d of %d", c, l, y, e.x, e.y, S.h); break; }
            }
        }
}

// the kernel's multiply-shift i -> i / n over i in [0, count): exact?  (distinct (n, inv, count) only: rigs repeat them)
static bool recip_exact(int n, unsigned inv, int count) {
    static std::set<std::tuple<int, unsigned, int> > seen;
    if (!seen.insert(std::make_tuple(n, inv, count)).second) return true;
    for (int i = 0; i < count; ++i) if ((int)(umul24((unsigned)i, inv) >> 20) != i / n) return false;
    return true;
}

// 3a. spans of the one-launch tile kernel (k_pyramid_tiled), one axis of one camera
static void check_spans1_axis(const Planned& P, int c, bool is_x, bool* halo_ok) {
    const PlanInput& in = P.in; const GeometryPlan& G = P.G; const int ML = in.max_levels, NL = in.cams[c].p.nlevels, T = G.pyr_tile;
    const int nt = is_x ? G.pyr_tx[c] : G.pyr_ty[c], no = is_x ? G.pyr_ty[c] : G.pyr_tx[c];
    auto LV = [&](int l) -> const LevelInfo& { return G.levels[(size_t)c * ML + l]; };
    auto dim = [&](int l) { return is_x ? LV(l).w : LV(l).h; };
    auto S = [&](int l, int k) { return is_x ? G.psx[((size_t)c * ML + l) * G.pyr_tx_max + k] : G.psy[((size_t)c * ML + l) * G.pyr_ty_max + k]; };
    auto O = [&](int l, int k) { return is_x ? G.psy[((size_t)c * ML + l) * G.pyr_ty_max + k] : G.psx[((size_t)c * ML + l) * G.pyr_tx_max + k]; };
    CHECK(nt == (dim(0) + T - 1) / T, "cam %d tiles", c);
    for (int l = 0; l < NL; ++l) {
        int other_max = 0;
        for (int k = 0; k < no; ++k) other_max = std::max(other_max, O(l, k).z - O(l, k).x);
        for (int k = 0; k < nt; ++k) {
            const plan_int4 s = S(l, k);
            // owned runs tile [0, dim) (stores: x:374, `yy < oh && xx < ow` at dst + y0 * stride + x0), owned within needed, needed within the level
            CHECK(s.x == (k == 0 ? 0 : S(l, k - 1).y) && (k + 1 < nt || s.y == dim(l)) && s.x <= s.y, "cam %d %c level %d tile %d owns [%d, %d)", c, is_x ? 'x' : 'y', l, k, s.x, s.y);
            CHECK(s.y <= s.z && s.z <= dim(l), "cam %d %c level %d tile %d owns to %d needs to %d of %d", c, is_x ? 'x' : 'y', l, k, s.y, s.z, dim(l));
            if (l == 0) {   // the kernel takes the tile's origin as k T and stages T + PYR_HALO of level 0 (x:239-250)
                CHECK(s.x == std::min(k * T, dim(0)), "cam %d level 0 tile %d starts at %d", c, k, s.x);
                if (s.z - s.x > T + PYR_HALO) *halo_ok = false;
                continue;
            }
            // every tap of every needed destination lies in the region of the level above (x:356-361: srcl[(row - py0) * ppw + column - px0])
            const plan_int4 u = S(l - 1, k);
            for (int d = s.x; d < s.z; ++d) {
                const int a = is_x ? x_tap0(G, LV(l), d) : G.yt[LV(l).ytab_off + d].x, b = is_x ? x_tap1(G, LV(l), d) : G.yt[LV(l).ytab_off + d].y;
                if (!(a >= u.x && b < u.z)) { CHECK(false, "cam %d %c level %d tile %d destination %d taps %d %d outside [%d, %d)", c, is_x ? 'x' : 'y', l, k, d, a, b, u.x, u.z); break; }
            }
            // .w of the x spans splits the flattened region index (x:347-355; the y spans' .w is not read by the kernel)
            const int nn = s.z - s.x;
            if (is_x && nn > 0) {
                CHECK((unsigned)s.w == ((1u << 20) + nn - 1) / nn, "cam %d level %d tile %d reciprocal", c, l, k);
                CHECK(recip_exact(nn, (unsigned)s.w, nn * other_max), "cam %d level %d tile %d: index / %d inexact below %d", c, l, k, nn, nn * other_max);
            }
        }
    }
}

static bool check_spans1(const Planned& P) {
    const PlanInput& in = P.in; const GeometryPlan& G = P.G; const int ML = in.max_levels, T = G.pyr_tile;
    bool halo_ok = true;
    for (int c = 0; c < in.n_cams; ++c) {
        if (in.cur_w[c] == 0 || in.cur_h[c] == 0) { CHECK(G.pyr_tx[c] == 0 && G.pyr_ty[c] == 0, "empty camera %d has tiles", c); continue; }   // x:219
        CHECK(G.pyr_tx[c] <= G.pyr_tx_max && G.pyr_ty[c] <= G.pyr_ty_max, "cam %d tile counts", c);
        check_spans1_axis(P, c, true, &halo_ok);
        check_spans1_axis(P, c, false, &halo_ok);
        // LDS of a tile: tab_cap row entries (int4) + tab_cap column entries (int2) + the regions, level after level (x:224-226, 341)
        for (int ky = 0; ky < G.pyr_ty[c]; ++ky)
            for (int kx = 0; kx < G.pyr_tx[c]; ++kx) {
                int bytes = (T + PYR_HALO) * (T + PYR_HALO), nx = 0, ny = 0;
                for (int l = 1; l < in.cams[c].p.nlevels; ++l) {
                    const plan_int4 X = G.psx[((size_t)c * ML + l) * G.pyr_tx_max + kx], Y = G.psy[((size_t)c * ML + l) * G.pyr_ty_max + ky];
                    const int nw = std::max(X.z - X.x, 0), nh = std::max(Y.z - Y.x, 0);
                    bytes += ((nw + 3) & ~3) * nh; nx += nw; ny += nh;
                }
                if (!(nx <= G.pyr_tab_cap && ny <= G.pyr_tab_cap && bytes + 24 * G.pyr_tab_cap <= G.pyr_lds)) { CHECK(false, "cam %d tile %d,%d: %d + %d entries, %d bytes; cap %d, LDS %d", c, kx, ky, nx, ny, bytes, G.pyr_tab_cap, G.pyr_lds); break; }
            }
    }
    return halo_ok;
}

// 3b. spans of the large-rig tile kernel (k_pyramid_tiled4), one axis of one camera in one of the two launches
static void check_spans4_axis(const Planned& P, const TilePlan& TP, int c, bool is_x) {
    const PlanInput& in = P.in; const GeometryPlan& G = P.G; const int ML = in.max_levels;
    const int NL = std::min(in.cams[c].p.nlevels - 1, TP.last), nt = is_x ? TP.tx[c] : TP.ty[c], tile = is_x ? TP.tw : TP.th, halo = is_x ? TP.halo_x : TP.halo_y;
    auto LV = [&](int l) -> const LevelInfo& { return G.levels[(size_t)c * ML + l]; };
    auto dim = [&](int l) { return is_x ? LV(l).w : LV(l).h; };
    auto ext = [&](int l) { return is_x && l > TP.base ? 4 * ((dim(l) + 3) / 4) : dim(l); };   // x below the base: whole groups of four (stores land in the row pitch's padding, x:534)
    auto S = [&](int l, int k) { return is_x ? TP.sx[((size_t)c * ML + l) * TP.tx_max + k] : TP.sy[((size_t)c * ML + l) * TP.ty_max + k]; };
    CHECK(nt == (dim(TP.base) + tile - 1) / tile && nt <= (is_x ? TP.tx_max : TP.ty_max), "cam %d tiles", c);
    for (int l = TP.base; l <= NL; ++l)
        for (int k = 0; k < nt; ++k) {
            const plan_int4 s = S(l, k);
            const char ax = is_x ? 'x' : 'y';
            CHECK(s.x == (k == 0 ? 0 : S(l, k - 1).y) && (k + 1 < nt || s.y == ext(l)) && s.x <= s.y, "cam %d %c level %d tile %d owns [%d, %d) of %d", c, ax, l, k, s.x, s.y, ext(l));
            CHECK(s.y <= s.z && s.z <= ext(l), "cam %d %c level %d tile %d owns to %d needs to %d of %d", c, ax, l, k, s.y, s.z, ext(l));
            if (l == TP.base) {   // the staged base block: origin k * tile, tile + halo wide / high, clipped to the level (x:435-439)
                CHECK(s.x == std::min(k * tile, dim(l)) && s.z - s.x <= tile + halo, "cam %d %c base tile %d: [%d, %d), tile %d halo %d", c, ax, k, s.x, s.z, tile, halo);
                continue;
            }
            if (is_x) CHECK(s.x % 4 == 0 && s.y % 4 == 0 && s.z % 4 == 0, "cam %d level %d tile %d: x spans are whole groups", c, l, k);   // x:493-494 (>> 2), 432-433 (dword stores)
            const plan_int4 u = S(l - 1, k);
            for (int d = s.x; d < s.z; ++d) {   // x:509-525 (columns c + selector of the staged row), x:519 (rows yt.x, yt.y - py0)
                const int dd = is_x ? std::min(d, LV(l).w - 1) : d;   // columns past the width repeat the last one (build_resize_groups)
                const int a = is_x ? x_tap0(G, LV(l), dd) : G.yt[LV(l).ytab_off + d].x, b = is_x ? x_tap1(G, LV(l), dd) : G.yt[LV(l).ytab_off + d].y;
                if (!(a >= u.x && b < u.z)) { CHECK(false, "cam %d %c level %d tile %d destination %d taps %d %d outside [%d, %d)", c, ax, l, k, d, a, b, u.x, u.z); break; }
                if (is_x && d % 4 == 0) {   // the group's record (x:479, 507-511): first tap, and the taps of its four columns within eight bytes of it (v_perm over two dwords)
                    const plan_int4 g0 = G.xg[3 * (size_t)(LV(l).xgrp_off + d / 4)];
                    bool in8 = g0.x == a;
                    for (int j = 0; j < 4; ++j) { const int dj = std::min(d + j, LV(l).w - 1); in8 = in8 && x_tap0(G, LV(l), dj) >= g0.x && x_tap1(G, LV(l), dj) <= g0.x + 7; }
                    if (!in8) { CHECK(false, "cam %d level %d group %d: taps outside the eight bytes from %d", c, l, d / 4, g0.x); break; }
                }
            }
            if (is_x) {   // .w: lane -> (row of the pass, group) for every lane, and NT -> rows per pass (x:503-505); every group needs a lane
                const int ngn = (s.z - s.x) / 4;
                if (ngn > 0) {
                    CHECK((unsigned)s.w == ((1u << 20) + ngn - 1) / ngn && ngn <= TP.threads, "cam %d level %d tile %d: %d groups, reciprocal %d", c, l, k, ngn, s.w);
                    CHECK(recip_exact(ngn, (unsigned)s.w, TP.threads + 1), "cam %d level %d tile %d: lane / %d inexact", c, l, k, ngn);
                }
            }
        }
}

static void check_spans4(const Planned& P) {
    const PlanInput& in = P.in; const GeometryPlan& G = P.G; const int ML = in.max_levels;
    for (int pi = 0; pi < 2; ++pi) {
        const TilePlan& TP = G.tp[pi];
        CHECK(TP.ok, "launch %d of a chosen plan is not ok", pi);
        if (TP.last <= TP.base) continue;
        CHECK(TP.last - TP.base + 1 <= PYR_MAX_LEVELS, "launch %d levels", pi);   // s_sx[PYR_MAX_LEVELS], x:408
        for (int c = 0; c < in.n_cams; ++c) {
            const LevelInfo& Lb = G.levels[(size_t)c * ML + TP.base];
            if (Lb.w == 0) { CHECK(TP.tx[c] == 0 && TP.ty[c] == 0, "launch %d: camera %d without the base level has tiles", pi, c); continue; }   // x:413
            check_spans4_axis(P, TP, c, true);
            check_spans4_axis(P, TP, c, false);
            const int NL = std::min(in.cams[c].p.nlevels - 1, TP.last);
            // LDS of a tile: 3 x gcap group entries, rcap row entries, the base block, the regions (x:418-420, 436-437, 496)
            for (int ky = 0; ky < TP.ty[c]; ++ky)
                for (int kx = 0; kx < TP.tx[c]; ++kx) {
                    int bytes = (TP.tw + TP.halo_x) * (TP.th + TP.halo_y), ng = 0, nr = 0;
                    for (int l = TP.base + 1; l <= NL; ++l) {
                        const plan_int4 X = TP.sx[((size_t)c * ML + l) * TP.tx_max + kx], Y = TP.sy[((size_t)c * ML + l) * TP.ty_max + ky];
                        const int w = std::max(X.z - X.x, 0), h = std::max(Y.z - Y.x, 0);
                        bytes += w * h; ng += w / 4; nr += h;
                    }
                    if (!(ng <= TP.gcap && nr <= TP.rcap && bytes + 48 * TP.gcap + 16 * TP.rcap <= TP.lds)) { CHECK(false, "launch %d cam %d tile %d,%d: %d groups %d rows %d bytes; caps %d %d, LDS %d", pi, c, kx, ky, ng, nr, bytes, TP.gcap, TP.rcap, TP.lds); break; }
                }
        }
    }
}

// 4. form selection, restated from the rules (orbx_debug_pyramid_form: 0 one tile launch, 3 two launches, 2 the generic chain)
static void check_form(const Planned& P, bool halo_ok) {
    const PlanInput& in = P.in; const GeometryPlan& G = P.G; const int ML = in.max_levels;
    long long px0 = 0; int nl_max = 0; bool v4 = true;
    for (int c = 0; c < in.n_cams; ++c) {
        px0 += (long long)in.cur_w[c] * in.cur_h[c]; nl_max = std::max(nl_max, in.cams[c].p.nlevels);
        for (int l = 1; l < in.cams[c].p.nlevels; ++l) {
            const LevelInfo &Ls = G.levels[(size_t)c * ML + l - 1], &Ld = G.levels[(size_t)c * ML + l];
            if (Ld.w > 0 && (long long)Ls.w * 10 > (long long)Ld.w * 16) v4 = false;
        }
    }
    CHECK(G.v4_ok == v4, "v4_ok %d", (int)G.v4_ok);
    CHECK(G.pyr_tile == (px0 <= 1500000 ? 32 : 64), "tile %d for %lld pixels", G.pyr_tile, px0);
    if (G.tiled_ok) CHECK(G.pyr_lds <= 60 * 1024 && halo_ok && ML <= PYR_MAX_LEVELS, "one-launch form chosen with LDS %d, halo %d", G.pyr_lds, (int)halo_ok);
    const bool fits1 = G.pyr_lds <= 60 * 1024 && halo_ok && ML <= PYR_MAX_LEVELS && in.max_w <= 32767 && in.max_h <= 32767;
    const bool large = v4 && (in.pyr_chain == 1 || (in.pyr_chain < 0 && px0 > 4000000ll));
    const bool exp_tiled = fits1 && !large && in.pyr_chain != 2;
    CHECK(G.tiled_ok == exp_tiled, "one-launch form %d, rules say %d", (int)G.tiled_ok, (int)exp_tiled);
    CHECK(G.generic_chain == (in.pyr_chain == 2), "generic_chain");
    const bool want4 = v4 && !exp_tiled && in.pyr_chain != 2 && nl_max >= 2 && ML <= PYR_MAX_LEVELS && in.t4_plan[0] >= 16 && in.t4_plan[0] % 4 == 0 && in.t4_plan[1] >= 8;
    if (!want4) CHECK(!G.tiled4, "large-rig form chosen outside its rules");
    else CHECK(G.tiled4 == (G.tp[0].ok && G.tp[1].ok), "large-rig form %d, launches ok %d %d", (int)G.tiled4, (int)G.tp[0].ok, (int)G.tp[1].ok);
    CHECK(!(G.tiled_ok && G.tiled4), "two forms chosen");   // the third, the generic chain, is what is left: form = tiled_ok ? 0 : tiled4 ? 3 : 2
    if (G.tiled4)
        for (int pi = 0; pi < 2; ++pi) {
            const TilePlan& TP = G.tp[pi];
            if (TP.last <= TP.base) continue;
            CHECK(TP.lds <= 64 * 1024 && TP.halo_x % 4 == 0 && TP.halo_x >= 0 && TP.halo_y >= 0, "launch %d: LDS %d halo %d %d", pi, TP.lds, TP.halo_x, TP.halo_y);
            CHECK((TP.tw + TP.halo_x) / 4 * (TP.th + TP.halo_y) <= T4_MAX_DW * TP.threads, "launch %d: base block of %d dwords", pi, (TP.tw + TP.halo_x) / 4 * (TP.th + TP.halo_y));   // held[T4_MAX_DW], x:438-450
        }
    CHECK(G.l0_on == (in.l0_optin && G.tiled4), "l0_on");
}

// 5. byte-identical plans from the same input
template <typename V> static bool same_vec(const V& a, const V& b) { return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(a[0])) == 0); }
static bool same_plan(const GeometryPlan& A, const GeometryPlan& B) {
    bool s = same_vec(A.levels, B.levels) && same_vec(A.cell_map, B.cell_map) && same_vec(A.xt, B.xt) && same_vec(A.yt, B.yt) && same_vec(A.xg, B.xg) &&
             same_vec(A.psx, B.psx) && same_vec(A.psy, B.psy) && same_vec(A.slot_blk, B.slot_blk);
    s = s && A.cell_h_max == B.cell_h_max && A.cell_px_max == B.cell_px_max && A.total_cells == B.total_cells && A.total_slots == B.total_slots &&
        A.pyr_tx_max == B.pyr_tx_max && A.pyr_ty_max == B.pyr_ty_max && A.pyr_lds == B.pyr_lds && A.pyr_tile == B.pyr_tile && A.pyr_tab_cap == B.pyr_tab_cap &&
        std::memcmp(A.pyr_tx, B.pyr_tx, sizeof A.pyr_tx) == 0 && std::memcmp(A.pyr_ty, B.pyr_ty, sizeof A.pyr_ty) == 0 &&
        A.tiled_ok == B.tiled_ok && A.v4_ok == B.v4_ok && A.generic_chain == B.generic_chain && A.tiled4 == B.tiled4 && A.l0_on == B.l0_on && A.total_sel_slots == B.total_sel_slots;
    for (int pi = 0; pi < 2; ++pi) {
        const TilePlan &a = A.tp[pi], &b = B.tp[pi];
        s = s && a.base == b.base && a.last == b.last && a.tw == b.tw && a.th == b.th && a.halo_x == b.halo_x && a.halo_y == b.halo_y && a.tx_max == b.tx_max && a.ty_max == b.ty_max &&
            a.gcap == b.gcap && a.rcap == b.rcap && a.lds == b.lds && a.threads == b.threads && a.ok == b.ok && std::memcmp(a.tx, b.tx, sizeof a.tx) == 0 &&
            std::memcmp(a.ty, b.ty, sizeof a.ty) == 0 && same_vec(a.sx, b.sx) && same_vec(a.sy, b.sy);
    }
    return s;
}

static int n_forms[4] = {0, 0, 0, 0};
static void check_rig(const Rig& r) {
    g_rig = r.name;
    Planned P, Q;
    plan(r, P);
    CHECK(P.rc == ORB_OK, "refused: %s", P.why.c_str());
    if (P.rc != ORB_OK) return;
    check_levels(P);
    check_tables(P);
    const bool halo_ok = check_spans1(P);
    check_form(P, halo_ok);
    if (P.G.tiled4) check_spans4(P);
    ++n_forms[P.G.tiled_ok ? 0 : P.G.tiled4 ? 3 : 2];
    plan(r, Q);
    plan(r, Q);   // (also into a plan that held one already)
    CHECK(Q.rc == ORB_OK && same_plan(P.G, Q.G), "planning twice differs");
}

static bool refused(const Rig& r, const char* text) {
    Planned P;
    plan(r, P);
    return P.rc == ORB_E_ARG && P.why.find(text) != std::string::npos;
}

int main() {
    const int sizes[4][2] = {{640, 480}, {752, 480}, {1280, 720}, {1920, 1080}};
    const int plans[5][3] = {{128, 64, 3}, {32, 16, 0}, {256, 24, 1}, {64, 64, 5}, {64, 32, 99}};
    std::vector<Rig> rigs;
    char name[128];
    for (const auto& s : sizes)
        for (int n = 1; n <= 8; ++n) { std::snprintf(name, sizeof name, "%d x %dx%d", n, s[0], s[1]); rigs.push_back(rig(name, n, s[0], s[1])); }
    for (float sf : {1.2f, 1.05f, 2.0f})   // (2.0: level steps above 1.6, not v4_ok; three levels so that the last one still holds a cell)
        for (int chain : {-1, 0, 1, 2})
            for (const auto& s : {sizes[0], sizes[2], sizes[3]})
                for (int n : {2, 8}) {
                    std::snprintf(name, sizeof name, "%d x %dx%d scale %.2f chain %d", n, s[0], s[1], sf, chain);
                    rigs.push_back(rig(name, n, s[0], s[1], params(sf == 2.0f ? 3 : 8, sf), chain));
                }
    for (int nl : {1, 2})
        for (int chain : {-1, 1, 2}) { std::snprintf(name, sizeof name, "%d-level set chain %d", nl, chain); rigs.push_back(rig(name, 2, 640, 480, params(nl), chain)); }
    for (const auto& tp : plans)
        for (float sf : {1.2f, 1.05f})
            for (const auto& s : {sizes[0], sizes[3]}) {
                std::snprintf(name, sizeof name, "plan %d,%d,%d on 2 x %dx%d scale %.2f", tp[0], tp[1], tp[2], s[0], s[1], sf);
                Rig r = rig(name, 2, s[0], s[1], params(8, sf), 1);
                for (int i = 0; i < 3; ++i) r.t4[i] = tp[i] > 0 ? tp[i] : r.t4[i];   // (0 = keep, as orbx_debug_pyramid_plan)
                r.l0 = true;
                rigs.push_back(r);
            }
    for (int chain : {-1, 0, 1, 2}) {
        Rig r;   // mixed sizes and parameter sets, an empty camera among live ones, created for a larger image than any it holds
        std::snprintf(name, sizeof name, "mixed rig chain %d", chain);
        r.name = name; r.chain = chain; r.max_w = 1920; r.max_h = 1200; r.l0 = true;
        r.p = {params(8), params(8, 1.2f, 2000), params(2), params(8), params(1), params(5, 1.4f, 500), params(8, 1.05f)};
        r.w = {640, 1920, 752, 0, 1280, 641, 333}; r.h = {480, 1080, 480, 0, 720, 479, 247};
        rigs.push_back(r);
    }
    for (const Rig& r : rigs) check_rig(r);
    g_rig = "forms";
    CHECK(n_forms[0] > 0 && n_forms[2] > 0 && n_forms[3] > 0, "the list reaches forms %d %d %d", n_forms[0], n_forms[2], n_forms[3]);

    // the smallest image whose last level still holds a 30-px cell, and one pixel below it in each dimension
    g_rig = "smallest image";
    int w_min = 0, h_min = 0;
    for (int w = 64; w < 640 && !w_min; ++w) { Planned P; plan(rig("w", 1, w, 480), P); if (P.rc == ORB_OK) w_min = w; }
    for (int h = 64; h < 480 && !h_min; ++h) { Planned P; plan(rig("h", 1, 640, h), P); if (P.rc == ORB_OK) h_min = h; }
    CHECK(w_min > 64 && h_min > 64, "smallest accepted %d x %d", w_min, h_min);
    if (w_min > 64 && h_min > 64) {
        std::snprintf(name, sizeof name, "smallest image %dx%d", w_min, h_min);
        check_rig(rig(name, 1, w_min, h_min));
        CHECK(refused(rig("w - 1", 1, w_min - 1, h_min), "too small for the 30-px detection grid"), "%d x %d is not refused", w_min - 1, h_min);
        CHECK(refused(rig("h - 1", 1, w_min, h_min - 1), "too small for the 30-px detection grid"), "%d x %d is not refused", w_min, h_min - 1);
    }
    g_rig = "wide level";
    CHECK(refused(rig("wide", 1, 4096 + 33, 480), "or level size outside the supported range"), "a level of %d columns is not refused", 4096 + 33);
    CHECK(refused(rig("high", 1, 640, 4096 + 33), "or level size outside the supported range"), "a level of %d rows is not refused", 4096 + 33);
    check_rig(rig("widest level", 1, 4096 + 32, 480));

    std::printf("san_plan: %zu rigs, forms %d / %d / %d, %d failures\n", rigs.size(), n_forms[0], n_forms[2], n_forms[3], bad);
    return bad ? 1 : 0;
}
