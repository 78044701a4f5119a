// Lane scheduler of the grouped forward (conv_fwd.hip).  Host only: no HIP types, compiles with a plain C++ compiler.
// A launch UNIT is one tile form's kernel over a contiguous slice of that form's items, on a LANE (0 = the caller's stream,
// the others = side streams of the library).  At first every form is one unit, dealt from static duration weights; launch
// kFwdCalibAt of a plan times every unit on its lane, and a later launch cuts and deals the units again from those durations.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <utility>
#include <vector>

namespace pleas {

// tuned on the GPU
constexpr int kFwdMaxUnits = 24;            // units of one plan (timing events per plan, bound of the slicing)
constexpr int kFwdCalibAt = 3;              // the launch of a plan that is timed
constexpr int kFwdCalibKept = 16;           // geometries whose measured units are remembered
constexpr double kFillerMinShare = 0.15;    // the form with the most items levels the lanes if it is this much of the total
constexpr int kFillerMinItemsPerLane = 8;   // ... and has this many items per lane
constexpr double kSliceAbove = 0.7;         // a unit longer than this much of a lane's fair share is cut
constexpr int kSliceMinItems = 64;          // ... if it has this many items
constexpr double kSliceTarget = 0.45;       // ... into slices of about this much of the fair share
constexpr int kSliceMaxParts = 4;           // ... at most this many

struct FwdUnit { int form, begin, count, lane; double ms; };
// What the scheduler reads of a plan: form f owns items [form_begin[f], form_begin[f] + form_count[f]), item k has the
// relative duration item_work[k] (0 for padding).
struct FwdFormItems { int n_forms; const int* form_begin; const int* form_count; const float* item_work; };

inline int least_loaded_lane(const std::vector<double>& load) {
    int best = 0;
    for (int l = 1; l < (int)load.size(); ++l)
        if (load[l] < load[best]) best = l;
    return best;
}

// longest-processing-time first over the units' expected durations: the longest unit is launched first and keeps the caller's
// stream (every lane is empty then, lane 0 is the first of them), every other unit goes to the lane that is least loaded so far
inline void fwd_deal_lanes(std::vector<FwdUnit>& units, int lanes) {
    std::stable_sort(units.begin(), units.end(), [](const FwdUnit& a, const FwdUnit& b) { return a.ms > b.ms; });
    std::vector<double> load(lanes, 0.0);
    for (FwdUnit& u : units) {
        u.lane = least_loaded_lane(load);
        load[u.lane] += u.ms;
    }
}

// Cuts unit u into one slice per entry of `share` with share[k] / sum(share) of u's work (slices of share 0 are left out);
// the slice's lane field is its index k.
inline void fwd_slice_by_work(const float* item_work, const FwdUnit& u, const std::vector<double>& share, std::vector<FwdUnit>& out) {
    double work = 0, want = 0;
    for (int i = 0; i < u.count; ++i) work += item_work[u.begin + i];
    for (double v : share) want += v;
    int begin = u.begin;
    double acc = 0, upto = 0;
    size_t final_slice = 0;          // the last slice with a share takes what rounding left over
    for (size_t k = 0; k < share.size(); ++k)
        if (share[k] > 0) final_slice = k;
    if (!(want > 0) || !(work > 0)) {      // nothing to divide by: the unit stays whole (on the first lane that wanted a share)
        out.push_back(FwdUnit{u.form, u.begin, u.count, (int)final_slice, u.ms});
        return;
    }
    for (size_t k = 0; k < share.size(); ++k) {
        upto += work * share[k] / want;
        int end = begin;
        while (end < u.begin + u.count && share[k] > 0 && (k == final_slice || acc + item_work[end] <= upto)) acc += item_work[end++];
        if (end == begin && share[k] > 0 && end < u.begin + u.count) acc += item_work[end++];
        if (end > begin)                   // never a slice without items (a 0-block grid is an invalid launch)
            out.push_back(FwdUnit{u.form, begin, end - begin, (int)k, u.ms * share[k] / want});
        begin = end;
    }
}

// every form's slices must tile [form_begin, form_begin + form_count) exactly, each with at least one item and a lane
inline bool fwd_units_cover(std::vector<FwdUnit> units, const FwdFormItems& P, int lanes) {
    std::sort(units.begin(), units.end(), [](const FwdUnit& a, const FwdUnit& b) { return a.form != b.form ? a.form < b.form : a.begin < b.begin; });
    size_t k = 0;
    for (int f = 0; f < P.n_forms; ++f) {
        int at = P.form_begin[f];
        for (; k < units.size() && units[k].form == f; at += units[k++].count)
            if (units[k].count <= 0 || units[k].lane < 0 || units[k].lane >= lanes || units[k].begin != at) return false;
        if (at != P.form_begin[f] + P.form_count[f]) return false;
    }
    return k == units.size();
}

// After the calibration launch (`units`: one per form, ms = its measured duration).  What the in-job timelines showed: a
// form with few long items (stride-2 layers, the 7 x 7 layers: 400 - 900 items for 512 workgroup slots) needs WALL time
// whatever runs beside it, while the form with the most items (1 x 1 layers with K <= 256: 20 000 short ones) soaks up
// whatever the chip has left.  So: (1) every form but that FILLER is cut into slices of equal work if it outlasts kSliceAbove
// of a lane's fair share, and the units are list-scheduled onto the least-loaded lane in ascending order of their form's
// item count -- low parallelism first; (2) the filler is cut into one slice per lane, sized so that all lanes end together,
// launched last on each.
// Returns false -- and leaves `units` as they were -- when the measurements are unusable (an event that failed to time:
// ms <= 0) or the result would not launch every item exactly once; the caller then keeps the static lanes.
inline bool fwd_schedule_measured(std::vector<FwdUnit>& units, const FwdFormItems& P, int lanes, int max_units) {
    double total = 0;
    for (const FwdUnit& u : units) {
        if (!(u.ms > 0)) return false;
        total += u.ms;
    }
    if (!(total > 0)) return false;
    const double fair = total / lanes;
    int filler = -1;
    for (size_t i = 0; i < units.size(); ++i)
        if (filler < 0 || units[i].count > units[filler].count) filler = (int)i;
    if (filler >= 0 && (units[filler].ms < kFillerMinShare * total || units[filler].count < kFillerMinItemsPerLane * lanes)) filler = -1;
    // (1) the other forms, long ones in equal slices
    std::vector<FwdUnit> rest;
    for (size_t ui = 0; ui < units.size(); ++ui) {
        if ((int)ui == filler) continue;
        const FwdUnit u = units[ui];
        int parts = (u.ms > kSliceAbove * fair && u.count >= kSliceMinItems)
                        ? (int)std::min<double>(kSliceMaxParts, std::ceil(u.ms / (kSliceTarget * fair))) : 1;
        const int room = max_units - lanes - (int)rest.size() - (int)(units.size() - ui - 1);   // `lanes` units are the filler's
        parts = std::max(1, std::min(parts, room));
        if (parts <= 1) rest.push_back(u);
        else fwd_slice_by_work(P.item_work, u, std::vector<double>(parts, 1.0), rest);
    }
    std::stable_sort(rest.begin(), rest.end(), [&](const FwdUnit& a, const FwdUnit& b) {
        return P.form_count[a.form] != P.form_count[b.form] ? P.form_count[a.form] < P.form_count[b.form] : a.ms > b.ms;
    });
    std::vector<double> load(lanes, 0.0);
    for (FwdUnit& u : rest) {
        u.lane = least_loaded_lane(load);
        load[u.lane] += u.ms;
    }
    // (2) the filler levels the lanes
    if (filler >= 0) {
        const FwdUnit f = units[filler];
        double sum = f.ms;
        for (double v : load) sum += v;
        const double level = sum / lanes;
        std::vector<double> share(lanes);
        for (int l = 0; l < lanes; ++l) share[l] = std::max(0.0, level - load[l]);
        fwd_slice_by_work(P.item_work, f, share, rest);      // .lane = slice index = the lane it levels
    }
    if (!fwd_units_cover(rest, P, lanes)) return false;
    units.swap(rest);
    return true;
}

// Measured units per layer-list geometry (the plan key without its workspace address, element 1): a new fitter on the same
// layers -- every job of a bench run -- starts from the lanes the previous one measured.
struct FwdCalibStore {
    std::vector<std::pair<std::vector<int64_t>, std::vector<FwdUnit>>> kept;
    static std::vector<int64_t> geometry(std::vector<int64_t> key) {
        if (key.size() > 1) key[1] = 0;
        return key;
    }
    const std::vector<FwdUnit>* find(const std::vector<int64_t>& key) const {      // the newest record of the geometry
        const std::vector<int64_t> geo = geometry(key);
        for (auto kv = kept.rbegin(); kv != kept.rend(); ++kv)
            if (kv->first == geo) return &kv->second;
        return nullptr;
    }
    void publish(const std::vector<int64_t>& key, const std::vector<FwdUnit>& units) {
        if (kept.size() >= (size_t)kFwdCalibKept) kept.erase(kept.begin());
        kept.emplace_back(geometry(key), units);
    }
};

}  // namespace pleas
