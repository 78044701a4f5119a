// Stand-alone check of csrc/resample_plan.hpp (the host plan and executor of pleas_image_resample), meant to be compiled with
// -fsanitize=address,undefined and run as a child process (tests/test_resample_host.py): builds and executes plans for the
// geometries of tests/resample_cases.py, for a ragged batch at unaligned offsets and for degenerate sizes, walks every table of
// every plan against the bounds it must respect, and asks for every refusal.  Prints RESAMPLE_PLAN_OK and exits 0, or says
// what failed and exits 1.  Includes nothing of the library but that header.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "resample_plan.hpp"

using namespace pleas::resample;

static int failures = 0;
#define EXPECT(cond, ...)                     \
    do {                                      \
        if (!(cond)) {                        \
            std::printf("FAILED %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);         \
            std::printf("\n");                \
            ++failures;                       \
        }                                     \
    } while (0)

struct Case {
    int H, W, Ho, Wo, y0, x0, h, w, resize;      // resize 0: resized crop of the box; else Resize(s) + centre window
};

static std::vector<int32_t> geom_of(const Case& c) {
    if (!c.resize) return {c.H, c.W, c.y0, c.x0, c.h, c.w, c.Ho, c.Wo, 0, 0};
    const int Hv = c.W <= c.H ? (int)((double)c.resize * c.H / c.W) : c.resize;
    const int Wv = c.W <= c.H ? c.resize : (int)((double)c.resize * c.W / c.H);
    return {c.H, c.W, 0, 0, c.H, c.W, Hv, Wv, (int)std::lround((Hv - c.Ho) / 2.0), (int)std::lround((Wv - c.Wo) / 2.0)};
}

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

// every table entry of a valid plan stays inside what it indexes
static void walk(const std::vector<int32_t>& plan, const std::vector<int32_t>& geom, const std::vector<int64_t>& off, int C) {
    const int32_t* p = plan.data();
    const int N = p[kHN], Ho = p[kHHo], Wo = p[kHWo];
    const int64_t src_bytes = pair64(p + kHSrcLo), ws_bytes = pair64(p + kHWsLo);
    EXPECT(p[kHWords] == (int32_t)plan.size(), "plan words %d vs %zu", p[kHWords], plan.size());
    std::vector<int> rows_seen, out_seen;
    for (int s = 0; s < N; ++s) {
        const int32_t* sm = p + p[kHOffSamples] + s * kSampleWords;
        const int32_t* g = geom.data() + s * kGeomWords;
        EXPECT(pair64(sm + kSSrcLo) == off[s], "sample %d source offset", s);
        EXPECT(sm[kSRow0] >= g[kGY0] && sm[kSRow0] + sm[kSRows] <= g[kGY0] + g[kGh], "sample %d rows leave the box", s);
        EXPECT(pair64(sm + kSSrcLo) + (int64_t)g[kGH] * g[kGW] * C <= src_bytes, "sample %d leaves src", s);
        EXPECT(pair64(sm + kSWsLo) >= 0 && pair64(sm + kSWsLo) + (int64_t)sm[kSRows] * Wo * C <= ws_bytes, "sample %d leaves ws", s);
        for (int x = 0; x < Wo; ++x) {
            const int lo = p[sm[kSOffHB] + 2 * x], n = p[sm[kSOffHB] + 2 * x + 1];
            EXPECT(n >= 1 && n <= sm[kSKsH] && lo >= g[kGX0] && lo + n <= g[kGX0] + g[kGw], "sample %d x %d taps [%d, +%d)", s, x, lo, n);
            int64_t sum = 0;
            for (int j = 0; j < n; ++j) sum += p[sm[kSOffHK] + (int64_t)x * sm[kSKsH] + j];
            EXPECT(std::llabs(sum - (1 << kPrecisionBits)) <= sm[kSKsH], "sample %d x %d coefficients sum to %lld", s, x, (long long)sum);
        }
        for (int y = 0; y < Ho; ++y) {
            const int lo = p[sm[kSOffVB] + 2 * y], n = p[sm[kSOffVB] + 2 * y + 1];
            EXPECT(n >= 1 && n <= sm[kSKsV] && lo >= 0 && lo + n <= sm[kSRows], "sample %d y %d taps [%d, +%d)", s, y, lo, n);
            int64_t sum = 0;
            for (int j = 0; j < n; ++j) sum += p[sm[kSOffVK] + (int64_t)y * sm[kSKsV] + j];
            EXPECT(std::llabs(sum - (1 << kPrecisionBits)) <= sm[kSKsV], "sample %d y %d coefficients sum to %lld", s, y, (long long)sum);
        }
        rows_seen.assign((size_t)sm[kSRows], 0);
        out_seen.assign((size_t)Ho, 0);
        for (int it = 0; it < p[kHItemsH]; ++it) {
            const int32_t* item = p + p[kHOffItemsH] + 3 * it;
            EXPECT(item[0] >= 0 && item[0] < N, "rows item %d names sample %d", it, item[0]);
            if (item[0] == s)
                for (int r = item[1]; r < item[1] + item[2]; ++r) {
                    EXPECT(r >= 0 && r < sm[kSRows], "rows item %d row %d", it, r);
                    if (r >= 0 && r < sm[kSRows]) ++rows_seen[(size_t)r];
                }
        }
        for (int it = 0; it < p[kHItemsV]; ++it) {
            const int32_t* item = p + p[kHOffItemsV] + 3 * it;
            EXPECT(item[0] >= 0 && item[0] < N, "planes item %d names sample %d", it, item[0]);
            if (item[0] == s)
                for (int y = item[1]; y < item[1] + item[2]; ++y) {
                    EXPECT(y >= 0 && y < Ho, "planes item %d row %d", it, y);
                    if (y >= 0 && y < Ho) ++out_seen[(size_t)y];
                }
        }
        for (int v : rows_seen) EXPECT(v == 1, "sample %d: a workspace row is written %d times", s, v);
        for (int v : out_seen) EXPECT(v == 1, "sample %d: an output row is written %d times", s, v);
    }
}

// plan + execute a batch of cases; returns the resampled bytes [N][Ho][Wo][C]
static std::vector<uint8_t> run(const std::vector<Case>& cases, int C, int Ho, int Wo, const std::vector<uint8_t>& flip, uint32_t seed,
                                int gap) {
    const int64_t N = (int64_t)cases.size();
    std::vector<int32_t> geom;
    std::vector<int64_t> off;
    int64_t at = gap;
    for (const Case& c : cases) {
        const std::vector<int32_t> g = geom_of(c);
        geom.insert(geom.end(), g.begin(), g.end());
        off.push_back(at);
        at += (int64_t)c.H * c.W * C + gap;
    }
    std::vector<uint8_t> src((size_t)at);      // exactly the bytes the plan is told of: one byte past is a sanitizer report
    for (auto& b : src) b = (uint8_t)(lcg(seed) >> 24);
    Layout L;
    const char* e = layout_of(geom.data(), N, Ho, Wo, L);
    EXPECT(!e, "layout refused: %s", e ? e : "");
    if (e) return {};
    std::vector<int32_t> plan((size_t)L.words);
    e = build_plan(geom.data(), off.data(), N, C, Ho, Wo, at, plan.data(), plan.size() * 4);
    EXPECT(!e, "plan refused: %s", e ? e : "");
    if (e) return {};
    EXPECT(!check_header(plan.data(), plan.size() * 4), "header refused");
    walk(plan, geom, off, C);
    std::vector<float> lut((size_t)C * 256);
    for (size_t i = 0; i < lut.size(); ++i) lut[i] = (float)(i % 256);
    std::vector<float> dst((size_t)(N * C * Ho * Wo), -1.0f);
    std::vector<uint8_t> u8((size_t)(N * Ho * Wo * C)), ws((size_t)pair64(plan.data() + kHWsLo));
    execute(src.data(), plan.data(), lut.data(), flip.empty() ? nullptr : flip.data(), dst.data(), u8.data(), ws.data());
    for (int64_t s = 0; s < N; ++s)
        for (int c = 0; c < C; ++c)
            for (int y = 0; y < Ho; ++y)
                for (int x = 0; x < Wo; ++x) {
                    const float f = dst[(size_t)(((s * C + c) * Ho + y) * Wo + x)];
                    EXPECT(f == (float)u8[(size_t)(((s * Ho + y) * Wo + x) * C + c)], "dst and dst_u8 differ at %lld %d %d %d", (long long)s, c, y, x);
                }
    // an unchanged size is the identity (coefficients 2^22 and 0)
    for (int64_t s = 0; s < N; ++s) {
        const Case& c = cases[(size_t)s];
        if (c.resize || c.h != Ho || c.w != Wo) continue;
        const bool fl = !flip.empty() && flip[(size_t)s];
        for (int y = 0; y < Ho; ++y)
            for (int x = 0; x < Wo; ++x)
                for (int ch = 0; ch < C; ++ch) {
                    const int xs = fl ? Wo - 1 - x : x;
                    EXPECT(u8[(size_t)(((s * Ho + y) * Wo + x) * C + ch)] == src[(size_t)(off[(size_t)s] + ((int64_t)(c.y0 + y) * c.W + c.x0 + xs) * C + ch)],
                           "identity broken at sample %lld", (long long)s);
                }
    }
    return u8;
}

static void refusals() {
    std::vector<int32_t> plan(1 << 16);
    const size_t bytes = plan.size() * 4;
    const int64_t off[1] = {0};
    auto refused = [&](std::vector<int32_t> g, int C, int Ho, int Wo, int64_t src_bytes, int64_t o = 0, size_t pb = 0) {
        const int64_t offs[1] = {o};
        const char* e = build_plan(g.data(), offs, 1, C, Ho, Wo, src_bytes, plan.data(), pb ? pb : bytes);
        return e != nullptr && plan[kHMagic] != kMagic;
    };
    const std::vector<int32_t> ok = {8, 6, 1, 1, 5, 4, 4, 4, 0, 0};
    EXPECT(!build_plan(ok.data(), off, 1, 3, 4, 4, 8 * 6 * 3, plan.data(), bytes), "a valid plan is refused");
    EXPECT(refused({8, 6, 4, 1, 5, 4, 4, 4, 0, 0}, 3, 4, 4, 144), "box past the bottom");
    EXPECT(refused({8, 6, 1, 3, 5, 4, 4, 4, 0, 0}, 3, 4, 4, 144), "box past the right edge");
    EXPECT(refused({8, 6, -1, 0, 5, 4, 4, 4, 0, 0}, 3, 4, 4, 144), "negative box origin");
    EXPECT(refused({8, 6, 0, 0, 0, 4, 4, 4, 0, 0}, 3, 4, 4, 144), "empty box");
    EXPECT(refused({8, 6, 0, 0, 8, 6, 4, 4, 1, 0}, 3, 4, 4, 144), "window past the virtual output");
    EXPECT(refused({8, 6, 0, 0, 8, 6, 4, 4, 0, -1}, 3, 4, 4, 144), "negative window origin");
    EXPECT(refused({8, 6, 0, 0, 8, 6, 0, 4, 0, 0}, 3, 4, 4, 144), "empty virtual output");
    EXPECT(refused({0, 6, 0, 0, 8, 6, 4, 4, 0, 0}, 3, 4, 4, 144), "empty image");
    EXPECT(refused({16385, 6, 0, 0, 8, 6, 4, 4, 0, 0}, 3, 4, 4, (int64_t)16385 * 6 * 3), "a side above 16384");
    EXPECT(refused({8, 6, 0, 0, 8, 6, 16385, 4, 0, 0}, 3, 4, 4, 144), "a virtual side above 16384");
    EXPECT(refused(ok, 0, 4, 4, 144) && refused(ok, 5, 4, 4, 144), "C outside 1 .. 4");
    EXPECT(refused(ok, 3, 0, 4, 144) && refused(ok, 3, 4, -2, 144), "non-positive output size");
    EXPECT(refused(ok, 3, 4, 4, 143), "src one byte short");
    EXPECT(refused(ok, 3, 4, 4, 144, 1), "offset + size past src");
    EXPECT(refused(ok, 3, 4, 4, 144, -1), "negative offset");
    EXPECT(refused(ok, 3, 4, 4, -1), "negative src size");
    EXPECT(refused(ok, 3, 4, 4, 144, 0, 64), "plan memory too small");
    EXPECT(build_plan(ok.data(), off, 1, 3, 4, 4, 144, nullptr, bytes) != nullptr, "null plan memory");
    EXPECT(build_plan(nullptr, off, 1, 3, 4, 4, 144, plan.data(), bytes) != nullptr, "null geometry");
    EXPECT(build_plan(ok.data(), nullptr, 1, 3, 4, 4, 144, plan.data(), bytes) != nullptr, "null offsets");
    EXPECT(build_plan(ok.data(), off, -1, 3, 4, 4, 144, plan.data(), bytes) != nullptr, "negative N");
    // an empty batch is a plan of its own
    EXPECT(!build_plan(nullptr, nullptr, 0, 3, 4, 4, 0, plan.data(), bytes) && plan[kHN] == 0 && !check_header(plan.data(), bytes), "N == 0");
    // headers a launch refuses
    EXPECT(!build_plan(ok.data(), off, 1, 3, 4, 4, 144, plan.data(), bytes), "a valid plan is refused");
    EXPECT(check_header(plan.data(), (size_t)plan[kHWords] * 4 - 4) != nullptr, "plan longer than plan_bytes");
    EXPECT(check_header(nullptr, bytes) != nullptr && check_header(plan.data(), 8) != nullptr, "null or short plan");
    plan[kHMagic] ^= 1;
    EXPECT(check_header(plan.data(), bytes) != nullptr, "wrong magic");
}

int main() {
    const Case cases[] = {{37, 53, 16, 24, 0, 0, 37, 53, 0}, {20, 31, 32, 32, 0, 0, 20, 31, 0},   {9, 7, 8, 8, 0, 0, 9, 7, 0},
                          {1, 1, 4, 4, 0, 0, 1, 1, 0},       {2, 3, 7, 5, 0, 0, 2, 3, 0},         {300, 17, 5, 40, 0, 0, 300, 17, 0},
                          {64, 64, 64, 32, 0, 0, 64, 64, 0}, {120, 90, 48, 32, 20, 10, 75, 60, 0}, {50, 37, 20, 20, 0, 0, 50, 37, 24},
                          {31, 64, 20, 20, 0, 0, 31, 64, 24}};
    uint32_t seed = 1;
    for (const Case& c : cases)
        for (int C : {1, 3, 4}) run({c}, C, c.Ho, c.Wo, {}, ++seed, 0);
    // ragged batches at offsets that are no multiple of 4, flipped and not; the last sample ends where src ends
    for (int C : {1, 2, 3, 4}) {
        run({{37, 53, 16, 16, 3, 5, 30, 41, 0}, {1, 1, 16, 16, 0, 0, 1, 1, 0}, {16, 16, 16, 16, 0, 0, 16, 16, 0}, {300, 17, 16, 16, 1, 0, 299, 17, 0},
             {21, 40, 16, 16, 2, 20, 16, 16, 0}},
            C, 16, 16, {1, 0, 1, 0, 1}, ++seed, 0);
        run({{50, 37, 20, 20, 0, 0, 50, 37, 24}, {31, 64, 20, 20, 0, 0, 31, 64, 24}, {24, 24, 20, 20, 0, 0, 24, 24, 24}}, C, 20, 20, {}, ++seed, 3);
    }
    // the largest sides the plan admits, down to one pixel and up from one
    run({{1, 16384, 1, 1, 0, 0, 1, 16384, 0}}, 1, 1, 1, {}, ++seed, 0);
    run({{16384, 1, 3, 2, 0, 0, 16384, 1, 0}}, 2, 3, 2, {1}, ++seed, 1);
    run({{1, 1, 1, 700, 0, 0, 1, 1, 0}}, 4, 1, 700, {}, ++seed, 0);
    refusals();
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("RESAMPLE_PLAN_OK\n");
    return 0;
}
