// What the translation units of a replayed SET of tracks share (replay_set.hip, replay_set_analysis.hip; DESIGN.md sections 26 to 28): the arguments
// every set kernel reads, a track's ReplayView built from its table entry, and the host checks of the track table (defined in replay_set.hip).
#pragma once
#include "wtk_internal.h"
#include "replay_device.h"

namespace wtk {

struct SetArgs {
    Geometry g; // x_max / y_max are each track's own
    const wtk_replay_set_track *tracks; // [T] on the device
    const wtk_replay_set_geometry *geom; // [T] on the device (nullable: g's camera and microscope for every track)
    int T, E, kind;
    int S; // chunks of all tracks
    const double *track; // the super-track
    const double *a, *b;
    const int *valid;
    const double *share;
    int *pos, *move;        // [n_super / L][E][2]
    double *partial;        // [E][S][kSummary]
    double *track_summary;  // [T][E][kSummary]
    double *summary;        // [E][kSummary]
    double *objective;      // [E] (nullable)
    double *track_objective; // [T][E] (nullable)
    int num, den;           // objective = slot num / slot den
    const int *stop;
};

// The ONE place a track's Geometry is made: the set's cycle structure, the track's own clamp and, where the set has a geometry table (DESIGN.md section
// 29), the track's own camera and microscope.  `t` is uniform wherever this is called, so the branch and the loads stay scalar.
__device__ __forceinline__ Geometry track_geometry(const SetArgs &a, int t, const wtk_replay_set_track &tr) {
    Geometry g = a.g;
    g.x_max = tr.x_max, g.y_max = tr.y_max;
    if (a.geom) {
        const wtk_replay_set_geometry tg = a.geom[t];
        g.cam_w = tg.cam_w, g.cam_h = tg.cam_h, g.mic_w = tg.mic_w, g.mic_h = tg.mic_h;
    }
    return g;
}

// track t (entry `tr`) of the set as a scanned population: the super-track and the scan's arrays from the track's offset on, the track's own geometry and counts
__device__ __forceinline__ ReplayView track_view(const SetArgs &a, int t, const wtk_replay_set_track &tr) {
    const long long c0 = (long long)tr.cyc_off * a.E;
    ReplayView v;
    v.g = track_geometry(a, t, tr), v.E = a.E, v.C = tr.n_cycles, v.n_log = tr.n_log, v.R = tr.R;
    v.track = a.track + 4 * (long long)tr.cyc_off * a.g.L, v.share = a.share, v.pos = a.pos + 2 * c0, v.move = a.move + 2 * c0;
    return v;
}

// The checks of the table every entry point shares: each track as replay_view sees it (reported with its index), the derived fields, the slots and
// guards.  Leaves the shared geometry in a.g, the chunk count in a.S and the smallest n_log in min_log.  geom_host / geom_dev: the per-track geometry
// table or both null; with it every track is checked with its own camera and microscope (a.g then holds the last track's: track_geometry overrides them).
int set_view(const char *who, const wtk_replay_config *cfg, const wtk_replay_set_track *host, const wtk_replay_set_track *dev,
             const wtk_replay_set_geometry *geom_host, const wtk_replay_set_geometry *geom_dev, int32_t T, int32_t guard_cycles,
             int32_t kind, int32_t E, const double *track_dev, int32_t n_super, const double *share_dev, const int32_t *pos_dev, const int32_t *move_dev, SetArgs &a,
             int &min_log);

} // namespace wtk
