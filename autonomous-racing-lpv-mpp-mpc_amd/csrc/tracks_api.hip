// tracks_api.hip -- C ABI of the per-vehicle tracks (include/lpvmpc.h, "Per-vehicle tracks"): the handle's palette of track tables
// with the palette entry of every vehicle, its checks and the read-back.  The binding acts through lpvmpc::launch_lpv / launch_abc
// (lpv_eval.hip), which every route that linearises calls with the handle's binding (lpvmpc_trk), through the two stand-alone
// transforms, the hand-off (cascade_api.hip), the lap-0 fleet started by lpvmpc_cl_init_tyres (lpvmpc_api.hip) and the race started by
// lpvmpc_race_init_tyres (race_api.hip); kernels: track_lpv_eval.hip, track_vehicles.hip, track_race.hip.
#include <algorithm>
#include <cmath>
#include <vector>

#include "lpvmpc_handle.hpp"

static_assert(lpvmpc::kMaxTracks == LPVMPC_MAX_TRACKS && lpvmpc::kMaxSeg == LPVMPC_MAX_TRACK_ROWS, "the palette's limits");

int lpvmpc_tracks_check(lpvmpc_handle *h, int B, const char *who) {
    if (h->trk.tab && h->trk.B != B)
        return fail(h, LPVMPC_E_ARG, "%s: B=%d, but the handle has tracks for %d vehicles bound (lpvmpc_set_tracks)", who, B, h->trk.B);
    return LPVMPC_OK;
}

int lpvmpc_tracks_unbound(lpvmpc_handle *h, const lpvmpc_handle *bound, const char *who, const char *general) {
    if (bound && bound->trk.tab && general)
        return fail(h, LPVMPC_E_ARG, "%s: a handle with per-vehicle tracks bound (lpvmpc_set_tracks) starts through %s only, the most general "
                    "entry point (with NULL rows it computes what this call computes); T = 0 unbinds", who, general);
    if (bound && bound->trk.tab)
        return fail(h, LPVMPC_E_ARG, "%s: a handle with per-vehicle tracks bound (lpvmpc_set_tracks) runs the transforms, the LPV calls, the "
                    "solves, the hand-off, the lap-0 fleet and the race; the cascade takes the handle's own track (T = 0 unbinds)", who);
    return LPVMPC_OK;
}

extern "C" int lpvmpc_set_tracks(lpvmpc_handle *h, int32_t T, const int32_t *track_rows, const double *tables, const double *half_width,
                                 const double *slack, int32_t B, const int32_t *track_of) {
    const char *who = "lpvmpc_set_tracks";
    if (!h) return fail(nullptr, LPVMPC_E_ARG, "%s: handle is NULL", who);
    if (busy(h))
        return fail(h, LPVMPC_E_ARG, "%s: this handle runs a %s; bind the tracks before it starts (lpvmpc_cl_release ends it)", who,
                    h->cl_plant ? "closed-loop fleet" : (h->race || h->race_owner) ? "race" : "planner + controller cascade");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (T == 0 || B == 0) {                                              // unbind (freeing the tables waits for the launches that read them)
        static_cast<TrackTable &>(*h) = TrackTable{};
        return LPVMPC_OK;
    }
    if (T < 1 || T > LPVMPC_MAX_TRACKS) return fail(h, LPVMPC_E_ARG, "%s: T=%d outside [1,%d] (0 unbinds)", who, T, LPVMPC_MAX_TRACKS);
    if (B < 0) return fail(h, LPVMPC_E_ARG, "%s: B=%d", who, B);
    if (!track_rows || !tables || !half_width || !slack || !track_of) return fail(h, LPVMPC_E_ARG, "%s: NULL array (T = 0 or B = 0 unbinds)", who);
    constexpr int S = LPVMPC_MAX_TRACK_ROWS * 6;
    TrackTable t;
    t.trk_tables.assign((size_t)T * S, 0.0);                             // the rows in use; the others stay zero on the device
    for (int k = 0; k < T; ++k) {
        const int rows = track_rows[k];
        if (rows < 2 || rows > LPVMPC_MAX_TRACK_ROWS)
            return fail(h, LPVMPC_E_ARG, "%s: track %d has track_rows=%d outside [2,%d]", who, k, rows, LPVMPC_MAX_TRACK_ROWS);
        for (int i = 0; i < rows * 6; ++i) {
            const double w = tables[(size_t)k * S + i];
            if (!std::isfinite(w)) return fail(h, LPVMPC_E_ARG, "%s: track %d, row %d, word %d is not finite", who, k, i / 6, i % 6);
            t.trk_tables[(size_t)k * S + i] = w;
        }
        for (int i = 0; i < rows; ++i)
            if (!(tables[(size_t)k * S + i * 6 + 4] > 0))
                return fail(h, LPVMPC_E_ARG, "%s: track %d, row %d has segment length %g (must be > 0)", who, k, i, tables[(size_t)k * S + i * 6 + 4]);
        if (!std::isfinite(half_width[k]) || half_width[k] < 0 || !std::isfinite(slack[k]) || slack[k] < 0)
            return fail(h, LPVMPC_E_ARG, "%s: track %d has half_width=%g, slack=%g (finite and >= 0)", who, k, half_width[k], slack[k]);
    }
    for (int b = 0; b < B; ++b)
        if (track_of[b] < 0 || track_of[b] >= T) return fail(h, LPVMPC_E_ARG, "%s: track_of[%d]=%d outside [0,%d]", who, b, track_of[b], T - 1);
    t.trk_rows.assign(track_rows, track_rows + T); t.trk_of.assign(track_of, track_of + B);
    t.trk_hw.assign(half_width, half_width + T); t.trk_slack.assign(slack, slack + T);
    // the handle's own vehicle words as a model table [7][B]: what the bound LPV / ABC kernels read on a handle without model rows
    std::vector<double> own((size_t)lpvmpc::kModelWords * B);
    const double w[lpvmpc::kModelWords] = {h->cfg.lf, h->cfg.lr, h->cfg.m, h->cfg.Iz, h->cfg.Cf, h->cfg.Cr, h->cfg.mu};
    for (int i = 0; i < lpvmpc::kModelWords; ++i) for (int b = 0; b < B; ++b) own[(size_t)i * B + b] = w[i];
    double *d_tab = nullptr, *d_hw = nullptr, *d_slack = nullptr;
    int32_t *d_rows = nullptr, *d_of = nullptr;
    HIP_TRY(h, t.trk_mem.alloc(d_tab, t.trk_tables.size() * 8));
    HIP_TRY(h, t.trk_mem.alloc(d_hw, (size_t)T * 8));
    HIP_TRY(h, t.trk_mem.alloc(d_slack, (size_t)T * 8));
    HIP_TRY(h, t.trk_mem.alloc(d_rows, (size_t)T * 4));
    HIP_TRY(h, t.trk_mem.alloc(d_of, (size_t)B * 4));
    HIP_TRY(h, t.trk_mem.alloc(t.d_trk_model, own.size() * 8));
    if (hipMemcpy(d_tab, t.trk_tables.data(), t.trk_tables.size() * 8, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_hw, t.trk_hw.data(), (size_t)T * 8, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_slack, t.trk_slack.data(), (size_t)T * 8, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_rows, t.trk_rows.data(), (size_t)T * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_of, t.trk_of.data(), (size_t)B * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(t.d_trk_model, own.data(), own.size() * 8, hipMemcpyHostToDevice) != hipSuccess)
        return fail(h, LPVMPC_E_HIP, "%s: uploading the tables failed", who);
    t.trk.tab = d_tab; t.trk.rows = d_rows; t.trk.hw = d_hw; t.trk.slack = d_slack; t.trk.of = d_of; t.trk.T = T; t.trk.B = B;
    static_cast<TrackTable &>(*h) = std::move(t);                        // (freeing the old tables waits for the launches that read them)
    return LPVMPC_OK;
}

// the binding as it was set: tables [T][LPVMPC_MAX_TRACK_ROWS * 6] with the rows beyond track_rows zero
extern "C" int lpvmpc_tracks_read(lpvmpc_handle *h, int32_t *T, int32_t *B, int32_t *track_rows, double *tables, double *half_width,
                                  double *slack, int32_t *track_of) {
    const char *who = "lpvmpc_tracks_read";
    if (!h) return fail(nullptr, LPVMPC_E_ARG, "%s: handle is NULL", who);
    if (!T || !B) return fail(h, LPVMPC_E_ARG, "%s: T / B is NULL", who);
    *T = h->trk.tab ? h->trk.T : 0; *B = h->trk.tab ? h->trk.B : 0;
    if (!h->trk.tab) return LPVMPC_OK;
    if (track_rows) std::copy(h->trk_rows.begin(), h->trk_rows.end(), track_rows);
    if (tables) std::copy(h->trk_tables.begin(), h->trk_tables.end(), tables);
    if (half_width) std::copy(h->trk_hw.begin(), h->trk_hw.end(), half_width);
    if (slack) std::copy(h->trk_slack.begin(), h->trk_slack.end(), slack);
    if (track_of) std::copy(h->trk_of.begin(), h->trk_of.end(), track_of);
    return LPVMPC_OK;
}
