// f1p_scene.hip -- what the planners plan against: the raceline's waypoints, the occupancy grid and its dilation, the footprint, the track set
#include "f1p_host.h"

using namespace f1p;

namespace f1p {

int need_tracks(f1p_ctx* ctx, bool psi, bool kappa) {
    if (ctx->trk_K < 1) return set_error(ctx, F1P_ESTATE, "no track set: call f1p_set_track_set first");
    if (psi && !ctx->trk_has_psi) return set_error(ctx, F1P_ESTATE, "the track set has no heading column");
    if (kappa && !ctx->trk_has_kappa) return set_error(ctx, F1P_ESTATE, "the track set has no curvature column");
    return F1P_OK;
}

}  // namespace f1p

// ---------------------------------------------------------------------------------------------------
int f1p_set_waypoints(f1p_ctx* ctx, const double* wp, int32_t n, int32_t ncols, int32_t col_x, int32_t col_y,
                      int32_t col_v, int32_t col_psi) {
    return f1p_set_waypoints_ex(ctx, wp, n, ncols, col_x, col_y, col_v, col_psi, -1);
}

// bounding box of every 64-segment chunk of the polyline (x, y) [n] (nearest_scan_boxed): box [ceil((n-1)/64)][4] = (xmin, xmax, ymin, ymax);
// infinite = "never skip this chunk".  The context's raceline and every track of a track set get their boxes from here.
static void chunk_boxes(const double* px, const double* py, int n, double* box) {
    const int nchunk = (n - 1 + 63) / 64;
    for (int c = 0; c < nchunk; ++c) {
        const int lo = 64 * c, hi = std::min(64 * c + 64, n - 1);
        double xmin = HUGE_VAL, xmax = -HUGE_VAL, ymin = HUGE_VAL, ymax = -HUGE_VAL;
        bool open_box = false;
        for (int i = lo; i <= hi; ++i) {
            const double x = px[i], y = py[i];
            if (!(fabs(x) <= 1.0e6) || !(fabs(y) <= 1.0e6)) open_box = true;
            if (i < hi) {
                const double dx = px[i + 1] - x, dy = py[i + 1] - y;
                if (!(dx * dx + dy * dy >= 1e-300)) open_box = true;   // zero-length (0/0 = NaN wins np.argmin) or NaN
            }
            xmin = std::min(xmin, x); xmax = std::max(xmax, x); ymin = std::min(ymin, y); ymax = std::max(ymax, y);
        }
        if (open_box) { xmin = ymin = -HUGE_VAL; xmax = ymax = HUGE_VAL; }
        box[4 * (size_t)c] = xmin; box[4 * (size_t)c + 1] = xmax; box[4 * (size_t)c + 2] = ymin; box[4 * (size_t)c + 3] = ymax;
    }
}

// largest finite |x|, |y| of a polyline (lookahead_slack, k_lattice_mixed.hip)
static double coord_absmax(const double* px, const double* py, size_t n) {
    double m = 0.0;
    for (size_t i = 0; i < n; ++i) {
        const double ax = fabs(px[i]), ay = fabs(py[i]);
        if (ax < HUGE_VAL && ax > m) m = ax;
        if (ay < HUGE_VAL && ay > m) m = ay;
    }
    return m;
}

int f1p_set_waypoints_ex(f1p_ctx* ctx, const double* wp, int32_t n, int32_t ncols, int32_t col_x, int32_t col_y,
                         int32_t col_v, int32_t col_psi, int32_t col_kappa) {
    F1P_ENTER(ctx);
    if (!wp) return set_error(ctx, F1P_EINVAL, "waypoints pointer is NULL");
    if (n < 2) return set_error(ctx, F1P_EINVAL, "at least 2 waypoints are required");
    if (ncols < 3) return set_error(ctx, F1P_EINVAL, "Waypoints needs to be a (Nxm), m >= 3, numpy array!");   // pure_pursuit.py:101-102
    auto bad = [&](int c) { return c < 0 || c >= ncols; };
    if (bad(col_x) || bad(col_y) || bad(col_v) || (col_psi >= 0 && bad(col_psi)) || (col_kappa >= 0 && bad(col_kappa)))
        return set_error(ctx, F1P_EINVAL, "column index out of range");
    std::vector<double> soa((size_t)5 * n, 0.0);
    if (col_psi >= 0)
        for (int i = 0; i < n; ++i) {
            const double psi = wp[(size_t)i * ncols + col_psi];
            if (!(psi >= -1.0e4 && psi <= 1.0e4)) return set_error(ctx, F1P_EINVAL, "waypoint heading must be finite and within +-1e4 rad");
        }
    for (int i = 0; i < n; ++i) {
        soa[i] = wp[(size_t)i * ncols + col_x];
        soa[(size_t)n + i] = wp[(size_t)i * ncols + col_y];
        soa[(size_t)2 * n + i] = wp[(size_t)i * ncols + col_v];
        soa[(size_t)3 * n + i] = col_psi >= 0 ? wp[(size_t)i * ncols + col_psi] : 0.0;
        soa[(size_t)4 * n + i] = col_kappa >= 0 ? wp[(size_t)i * ncols + col_kappa] : 0.0;
    }
    const int nchunk = (n - 1 + 63) / 64;
    std::vector<double> box((size_t)4 * nchunk);
    chunk_boxes(soa.data(), soa.data() + n, n, box.data());
    F1P_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->wp_gen++;                                                  // (the arc table of the rivals' prediction is the old raceline's)
    if (n != ctx->n_wp) {
        double** ps[] = {&ctx->d_wx, &ctx->d_wy, &ctx->d_wv, &ctx->d_wpsi, &ctx->d_wkappa, &ctx->d_wbox};
        for (double** p : ps) { if (*p) (void)hipFree(*p); *p = nullptr; }
        ctx->n_wp = 0;
        for (double** p : ps)
            F1P_HIP(ctx, hipMalloc((void**)p, sizeof(double) * (p == &ctx->d_wbox ? (size_t)4 * nchunk : (size_t)n)));
    }
    F1P_HIP(ctx, hipMemcpy(ctx->d_wbox, box.data(), sizeof(double) * box.size(), hipMemcpyHostToDevice));
    const size_t b = sizeof(double) * (size_t)n;
    F1P_HIP(ctx, hipMemcpy(ctx->d_wx, soa.data(), b, hipMemcpyHostToDevice));
    F1P_HIP(ctx, hipMemcpy(ctx->d_wy, soa.data() + n, b, hipMemcpyHostToDevice));
    F1P_HIP(ctx, hipMemcpy(ctx->d_wv, soa.data() + 2 * (size_t)n, b, hipMemcpyHostToDevice));
    F1P_HIP(ctx, hipMemcpy(ctx->d_wpsi, soa.data() + 3 * (size_t)n, b, hipMemcpyHostToDevice));
    F1P_HIP(ctx, hipMemcpy(ctx->d_wkappa, soa.data() + 4 * (size_t)n, b, hipMemcpyHostToDevice));
    ctx->n_wp = n;
    ctx->wp_absmax = coord_absmax(soa.data(), soa.data() + n, (size_t)n);
    ctx->has_psi = col_psi >= 0;
    ctx->has_kappa = col_kappa >= 0;
    return F1P_OK;
}

static void drop_grid(f1p_ctx* ctx) {
    if (ctx->d_bits) (void)hipFree(ctx->d_bits);
    if (ctx->d_bits0) (void)hipFree(ctx->d_bits0);
    if (ctx->d_bits_clear) (void)hipFree(ctx->d_bits_clear);
    ctx->d_bits_clear = nullptr; ctx->clear_dist = 0.0;
    ctx->d_bits = nullptr; ctx->d_bits0 = nullptr; ctx->has_grid = false; ctx->inflate_radius = 0.0; ctx->user_inflate = 0.0; ctx->disc_radius = 0.0; ctx->n_disc = 0;
}

int f1p_set_grid(f1p_ctx* ctx, const uint8_t* img, int32_t w, int32_t h, double res, double ox, double oy,
                 int32_t occupied_below) {
    F1P_ENTER(ctx);
    if (!img) {   // clear
        F1P_HIP(ctx, hipStreamSynchronize(ctx->stream));
        drop_grid(ctx);
        return F1P_OK;
    }
    if (w < 1 || h < 1 || w > 65535 || h > 65535) return set_error(ctx, F1P_EINVAL, "grid size out of range");
    if (!(res > 0.0)) return set_error(ctx, F1P_EINVAL, "resolution must be > 0");
    F1P_HIP(ctx, hipStreamSynchronize(ctx->stream));
    drop_grid(ctx);
    ctx->gw = w; ctx->gh = h; ctx->gwwords = (w + 31) / 32;
    ctx->res = res; ctx->inv_res = 1.0 / res; ctx->ox = ox; ctx->oy = oy;
    const size_t bit_bytes = sizeof(uint32_t) * (size_t)ctx->gwwords * h;
    uint8_t* d_img = nullptr;
    F1P_HIP(ctx, hipMalloc((void**)&d_img, (size_t)w * h));
    int rc = check_hip(ctx, hipMalloc((void**)&ctx->d_bits0, bit_bytes), "hipMalloc(bits)");
    if (rc == F1P_OK) rc = check_hip(ctx, hipMalloc((void**)&ctx->d_bits, bit_bytes), "hipMalloc(bits)");
    if (rc == F1P_OK) rc = check_hip(ctx, hipMemcpyAsync(d_img, img, (size_t)w * h, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync(img)");
    if (rc == F1P_OK) rc = launch_pack_grid(ctx, d_img, w, h, occupied_below);
    if (rc == F1P_OK) rc = check_hip(ctx, hipMemcpyAsync(ctx->d_bits, ctx->d_bits0, bit_bytes, hipMemcpyDeviceToDevice, ctx->stream), "hipMemcpyAsync(bits)");
    if (rc == F1P_OK) rc = check_hip(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    (void)hipFree(d_img);
    if (rc != F1P_OK) { drop_grid(ctx); return rc; }
    ctx->has_grid = true;
    return F1P_OK;
}

static int edt_cap_check(f1p_ctx* ctx, int64_t cap) {
    if (!ctx->has_grid) return set_error(ctx, F1P_ESTATE, "occupancy grid not set: call f1p_set_grid first");
    if (cap < 1 || cap > 8192) return set_error(ctx, F1P_EINVAL, "distance cap must be within 1..8192 cells");
    return F1P_OK;
}

int f1p_grid_distance_batch(f1p_ctx* ctx, float* dist, int32_t cap_cells) {
    F1P_ENTER(ctx);
    if (!dist) return set_error(ctx, F1P_EINVAL, "dist is NULL");
    int rc = edt_cap_check(ctx, cap_cells);
    if (rc) return rc;
    const size_t n = (size_t)ctx->gw * ctx->gh;
    float* d_dist = nullptr;
    F1P_HIP(ctx, hipMalloc((void**)&d_dist, sizeof(float) * n));
    rc = launch_grid_edt(ctx, cap_cells, 0u, d_dist, nullptr, nullptr);
    if (rc == F1P_OK) rc = check_hip(ctx, hipMemcpy(dist, d_dist, sizeof(float) * n, hipMemcpyDeviceToHost), "hipMemcpy(dist)");
    (void)hipFree(d_dist);
    return rc;
}

// the active bitmap = the uploaded grid dilated by ONE disc of radius user_inflate + disc_radius (exact Euclidean distance
// transform, k_grid.hip): the user's inflation and the footprint's disc radius add, neither replaces the other
static int apply_dilation(f1p_ctx* ctx, double radius) {
    F1P_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->clear_dist = 0.0;                                  // the active bitmap changes: its clearance map is stale
    if (radius == 0.0) {
        F1P_HIP(ctx, hipMemcpy(ctx->d_bits, ctx->d_bits0, sizeof(uint32_t) * (size_t)ctx->gwwords * ctx->gh, hipMemcpyDeviceToDevice));
        ctx->inflate_radius = 0.0;
        return F1P_OK;
    }
    const double q = radius * ctx->inv_res;
    const double thr = ceil(q * q);                       // integer d2 < q^2  <=>  d2 < ceil(q^2)
    const int64_t cap = (int64_t)ceil(q) + 1;
    int rc = edt_cap_check(ctx, cap);
    if (rc) return rc;
    rc = launch_grid_edt(ctx, (int)cap, (uint32_t)thr, nullptr, nullptr, ctx->d_bits);
    if (rc == F1P_OK) ctx->inflate_radius = radius;
    return rc;
}

int f1p_inflate_grid(f1p_ctx* ctx, double radius) {
    F1P_ENTER(ctx);
    if (!ctx->has_grid) return set_error(ctx, F1P_ESTATE, "occupancy grid not set: call f1p_set_grid first");
    if (!(radius >= 0.0) || !isfinite(radius)) return set_error(ctx, F1P_EINVAL, "inflation radius must be finite and >= 0");
    const int rc = apply_dilation(ctx, radius + ctx->disc_radius);
    if (rc == F1P_OK) ctx->user_inflate = radius;
    return rc;
}

int f1p_set_footprint(f1p_ctx* ctx, int32_t n_discs, const double* offsets, double radius) {
    F1P_ENTER(ctx);
    if (n_discs < 0 || n_discs > 4 || (n_discs > 0 && !offsets)) return set_error(ctx, F1P_EINVAL, "between 0 and 4 footprint discs are supported");
    if (!ctx->has_grid) return set_error(ctx, F1P_ESTATE, "occupancy grid not set: call f1p_set_grid first");
    if (n_discs > 0 && (!(radius >= 0.0) || !isfinite(radius))) return set_error(ctx, F1P_EINVAL, "footprint disc radius must be finite and >= 0");
    for (int d = 0; d < n_discs; ++d)
        if (!isfinite(offsets[d]) || fabs(offsets[d]) > 100.0) return set_error(ctx, F1P_EINVAL, "footprint offsets must be finite and within +-100 m");
    const double disc = n_discs > 0 ? radius : 0.0;
    int rc = apply_dilation(ctx, ctx->user_inflate + disc);           // the disc radius adds to the user's inflation; n_discs = 0 restores it
    if (rc) return rc;
    ctx->disc_radius = disc;
    ctx->n_disc = n_discs;
    for (int d = 0; d < 4; ++d) ctx->disc_off[d] = d < n_discs ? offsets[d] : 0.0;
    return F1P_OK;
}

// test hooks (read-only): the packed maps cell by cell, and the point test on the active bitmap
int f1p_grid_debug_read(f1p_ctx* ctx, int32_t which, uint8_t* cells, double* clear_dist_cells, int32_t* padding_all_set) {
    F1P_ENTER(ctx);
    if (which < 0 || which > 2) return set_error(ctx, F1P_EINVAL, "which must be 0 (uploaded), 1 (active) or 2 (clearance)");
    if (!cells) return set_error(ctx, F1P_EINVAL, "cells is NULL");
    if (!ctx->has_grid) return set_error(ctx, F1P_ESTATE, "occupancy grid not set: call f1p_set_grid first");
    if (which == 2 && (!ctx->d_bits_clear || ctx->clear_dist == 0.0))
        return set_error(ctx, F1P_ESTATE, "no clearance map of the active bitmap: none was built yet, or the bitmap changed since (stale)");
    F1P_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int w = ctx->gw, h = ctx->gh, ww = ctx->gwwords;
    const uint32_t* src = which == 0 ? ctx->d_bits0 : which == 1 ? ctx->d_bits : ctx->d_bits_clear;
    std::vector<uint32_t> words((size_t)ww * h);
    F1P_HIP(ctx, hipMemcpy(words.data(), src, sizeof(uint32_t) * words.size(), hipMemcpyDeviceToHost));
    uint32_t pad_and = 0xffffffffu;
    const uint32_t pad_mask = (w & 31) ? ~((1u << (w & 31)) - 1u) : 0u;      // the bits of a row's last word beyond column w
    for (int gy = 0; gy < h; ++gy) {
        const uint32_t* row = words.data() + (size_t)gy * ww;
        uint8_t* dst = cells + (size_t)(h - 1 - gy) * w;                     // image row order: row 0 = top
        for (int gx = 0; gx < w; ++gx) dst[gx] = (uint8_t)((row[gx >> 5] >> (gx & 31)) & 1u);
        pad_and &= row[ww - 1] | ~pad_mask;
    }
    if (padding_all_set) *padding_all_set = pad_and == 0xffffffffu ? 1 : 0;
    if (clear_dist_cells) *clear_dist_cells = ctx->d_bits_clear ? ctx->clear_dist : 0.0;
    return F1P_OK;
}

int f1p_grid_occupied_batch(f1p_ctx* ctx, const double* pts, int32_t E, uint8_t* out) {
    F1P_ENTER(ctx);
    if (E < 0) return set_error(ctx, F1P_EINVAL, "E must be >= 0");
    if (E == 0) return F1P_OK;
    if (!pts || !out) return set_error(ctx, F1P_EINVAL, "pts or out is NULL");
    if (!ctx->has_grid) return set_error(ctx, F1P_ESTATE, "occupancy grid not set: call f1p_set_grid first");
    Stage s(ctx);
    s.need(sizeof(double) * 2 * (size_t)E); s.need((size_t)E);
    int rc = s.begin(); if (rc) return rc;
    const double* d_pts;
    if ((rc = s.in(pts, (size_t)2 * E, &d_pts))) return rc;
    uint8_t* d_out = s.out(out, (size_t)E);
    if ((rc = launch_grid_occupied(ctx, d_pts, E, d_out))) return rc;
    return s.finish();
}

// ---------------------------------------------------------------------------------------------------
// track set: K polylines, each ego follows the one its track id names (k_tracks.hip)
static void drop_track_set(f1p_ctx* ctx) {
    double** ps[] = {&ctx->d_tx, &ctx->d_ty, &ctx->d_tv, &ctx->d_tpsi, &ctx->d_tkappa, &ctx->d_tbox};
    for (double** p : ps) { if (*p) (void)hipFree(*p); *p = nullptr; }
    if (ctx->d_ttab) (void)hipFree(ctx->d_ttab);
    ctx->d_ttab = nullptr;
    ctx->trk_K = 0; ctx->trk_rows = 0; ctx->trk_chunks = 0; ctx->trk_has_psi = false; ctx->trk_has_kappa = false; ctx->trk_absmax = 0.0;
}

int f1p_set_track_set(f1p_ctx* ctx, const double* wp, const int64_t* row_offsets, int32_t K, int32_t ncols, int32_t col_x, int32_t col_y,
                      int32_t col_v, int32_t col_psi, int32_t col_kappa) {
    F1P_ENTER(ctx);
    if (K < 0) return set_error(ctx, F1P_EINVAL, "K must be >= 0");
    if (K == 0) {                                                   // clear
        F1P_HIP(ctx, hipStreamSynchronize(ctx->stream));
        ctx->trk_gen++;
        drop_track_set(ctx);
        return F1P_OK;
    }
    if (!wp || !row_offsets) return set_error(ctx, F1P_EINVAL, "waypoints and row offsets are required");
    if (ncols < 3) return set_error(ctx, F1P_EINVAL, "Waypoints needs to be a (Nxm), m >= 3, numpy array!");   // pure_pursuit.py:101-102
    auto bad = [&](int c) { return c < 0 || c >= ncols; };
    if (bad(col_x) || bad(col_y) || bad(col_v) || (col_psi >= 0 && bad(col_psi)) || (col_kappa >= 0 && bad(col_kappa)))
        return set_error(ctx, F1P_EINVAL, "column index out of range");
    if (row_offsets[0] != 0) return set_error(ctx, F1P_EINVAL, "row_offsets[0] must be 0");
    int64_t nchunk_all = 0;
    for (int k = 0; k < K; ++k) {
        const int64_t n = row_offsets[k + 1] - row_offsets[k];
        if (!(row_offsets[k + 1] > row_offsets[k]) || n < 2) return set_error(ctx, F1P_EINVAL, "row offsets must increase by at least 2 rows per track");
        if (row_offsets[k + 1] >= ((int64_t)1 << 31)) return set_error(ctx, F1P_EINVAL, "a track set holds fewer than 2^31 rows");
        nchunk_all += (n - 1 + 63) / 64;
    }
    const int64_t rows = row_offsets[K];
    if (col_psi >= 0)
        for (int64_t i = 0; i < rows; ++i) {
            const double psi = wp[(size_t)i * ncols + col_psi];
            if (!(psi >= -1.0e4 && psi <= 1.0e4)) return set_error(ctx, F1P_EINVAL, "waypoint heading must be finite and within +-1e4 rad");
        }
    // everything validated: the previous set stays in place until the new one is complete on the device
    std::vector<double> soa((size_t)5 * rows, 0.0);
    for (int64_t i = 0; i < rows; ++i) {
        const double* r = wp + (size_t)i * ncols;
        soa[i] = r[col_x];
        soa[(size_t)rows + i] = r[col_y];
        soa[(size_t)2 * rows + i] = r[col_v];
        soa[(size_t)3 * rows + i] = col_psi >= 0 ? r[col_psi] : 0.0;
        soa[(size_t)4 * rows + i] = col_kappa >= 0 ? r[col_kappa] : 0.0;
    }
    std::vector<double> box((size_t)4 * nchunk_all);
    std::vector<int32_t> tab((size_t)4 * K);
    int64_t c0 = 0;
    for (int k = 0; k < K; ++k) {
        const int64_t off = row_offsets[k], n = row_offsets[k + 1] - off;
        chunk_boxes(soa.data() + off, soa.data() + rows + off, (int)n, box.data() + 4 * c0);   // the rule of the context's raceline
        tab[4 * (size_t)k] = (int32_t)off; tab[4 * (size_t)k + 1] = (int32_t)n; tab[4 * (size_t)k + 2] = (int32_t)c0; tab[4 * (size_t)k + 3] = 0;
        c0 += (n - 1 + 63) / 64;
    }
    double* d[6] = {};
    int32_t* d_tab = nullptr;
    auto release = [&]() { for (double* p : d) if (p) (void)hipFree(p); if (d_tab) (void)hipFree(d_tab); };
    int rc = F1P_OK;
    for (int c = 0; c < 5 && rc == F1P_OK; ++c) {
        rc = check_hip(ctx, hipMalloc((void**)&d[c], sizeof(double) * (size_t)rows), "hipMalloc(track set)");
        if (rc == F1P_OK) rc = check_hip(ctx, hipMemcpy(d[c], soa.data() + (size_t)c * rows, sizeof(double) * (size_t)rows, hipMemcpyHostToDevice), "hipMemcpy(track set)");
    }
    if (rc == F1P_OK) rc = check_hip(ctx, hipMalloc((void**)&d[5], sizeof(double) * box.size()), "hipMalloc(track boxes)");
    if (rc == F1P_OK) rc = check_hip(ctx, hipMemcpy(d[5], box.data(), sizeof(double) * box.size(), hipMemcpyHostToDevice), "hipMemcpy(track boxes)");
    if (rc == F1P_OK) rc = check_hip(ctx, hipMalloc((void**)&d_tab, sizeof(int32_t) * tab.size()), "hipMalloc(track table)");
    if (rc == F1P_OK) rc = check_hip(ctx, hipMemcpy(d_tab, tab.data(), sizeof(int32_t) * tab.size(), hipMemcpyHostToDevice), "hipMemcpy(track table)");
    if (rc == F1P_OK) rc = check_hip(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");   // no launch still reads the old set
    if (rc != F1P_OK) { release(); return rc; }
    ctx->trk_gen++;                                                 // (the arc tables of the rivals' prediction are the old set's)
    drop_track_set(ctx);
    ctx->d_tx = d[0]; ctx->d_ty = d[1]; ctx->d_tv = d[2]; ctx->d_tpsi = d[3]; ctx->d_tkappa = d[4]; ctx->d_tbox = d[5]; ctx->d_ttab = d_tab;
    ctx->trk_K = K; ctx->trk_rows = (int)rows; ctx->trk_chunks = (int)nchunk_all;
    ctx->trk_absmax = coord_absmax(soa.data(), soa.data() + rows, (size_t)rows);
    ctx->trk_has_psi = col_psi >= 0;
    ctx->trk_has_kappa = col_kappa >= 0;
    return F1P_OK;
}
