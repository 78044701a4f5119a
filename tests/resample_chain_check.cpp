// Stand-alone check of the chain code of csrc/resample_plan.hpp (the host plan and executor of pleas_image_resample_chain), meant
// to be compiled with -fsanitize=address,undefined and run as a child process (tests/test_resample_chain_host.py): builds and
// executes chain plans for the geometries of tests/resample_chain_cases.py, alone and as ragged batches at unaligned offsets,
// and for degenerate sizes; walks every table of every plan against the bounds it must respect; compares the result with the two
// single-stage plans run one after the other; asks for every refusal and damages every header.  Prints RESAMPLE_CHAIN_OK and
// exits 0, or says what failed and exits 1.  Includes nothing of the library but that header.
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
    int H, W, H1, W1, y0, x0, h, w;
};

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

// every entry of a valid chain plan stays inside what it indexes, and every scratch row and output row has one writer
static void walk(const std::vector<int32_t>& plan, const std::vector<Case>& cases, const std::vector<int64_t>& off, int C) {
    const int32_t* p = plan.data();
    const int N = p[kCN];
    EXPECT(p[kCWords] == (int32_t)plan.size(), "plan words %d vs %zu", p[kCWords], plan.size());
    const int32_t* p1 = p + p[kCOff1];
    const int32_t* p2 = p + p[kCOff2];
    const int64_t src_bytes = pair64(p + kCSrcLo), ws_bytes = pair64(p + kCWsLo), mid_at = pair64(p + kCMidAtLo), mid_bytes = pair64(p + kCMidLo),
                  ws2_at = pair64(p + kCWs2AtLo);
    EXPECT(mid_at % 16 == 0 && ws2_at % 16 == 0 && mid_at + mid_bytes <= ws2_at && ws2_at + pair64(p2 + kHWsLo) == ws_bytes, "workspace regions");
    EXPECT(pair64(p1 + kHWsLo) == mid_at && p1[kHWords] == p[kCOff2] - p[kCOff1], "stage-1 section header");
    int64_t mid_next = 0;
    for (int s = 0; s < N; ++s) {
        const Case& c = cases[(size_t)s];
        const int32_t* sm = p1 + p1[kHOffSamples] + s * kSampleWords;
        const int32_t* sm2 = p2 + p2[kHOffSamples] + s * kSampleWords;
        EXPECT(pair64(sm + kSSrcLo) == off[(size_t)s] && pair64(sm + kSSrcLo) + (int64_t)c.H * c.W * C <= src_bytes, "sample %d leaves src", s);
        EXPECT(sm[kSW] == c.W && sm[kSWo] == c.w, "sample %d widths", s);
        EXPECT(sm[kSRow0] >= 0 && sm[kSRows] >= 1 && sm[kSRow0] + sm[kSRows] <= c.H, "sample %d rows leave the image", s);
        EXPECT(pair64(sm + kSWsLo) >= 0 && pair64(sm + kSWsLo) + (int64_t)sm[kSRows] * c.w * C <= mid_at, "sample %d leaves the stage-1 scratch", s);
        EXPECT(pair64(sm + kSMidLo) == mid_next && pair64(sm2 + kSSrcLo) == mid_next, "sample %d place in the intermediate", s);
        mid_next += (int64_t)c.h * c.w * C;
        EXPECT(sm2[kSW] == c.w && sm2[kSRow0] >= 0 && sm2[kSRow0] + sm2[kSRows] <= c.h, "sample %d stage 2 leaves the intermediate", s);
        for (int x = 0; x < c.w; ++x) {
            const int lo = p1[sm[kSOffHB] + 2 * x], n = p1[sm[kSOffHB] + 2 * x + 1];
            EXPECT(n >= 1 && n <= sm[kSKsH] && lo >= 0 && lo + n <= c.W, "sample %d x %d taps [%d, +%d)", s, x, lo, n);
            int64_t sum = 0;
            for (int j = 0; j < n; ++j) sum += p1[sm[kSOffHK] + (int64_t)x * sm[kSKsH] + j];
            EXPECT(std::llabs(sum - (1 << kPrecisionBits)) <= sm[kSKsH], "sample %d x %d coefficients sum to %lld", s, x, (long long)sum);
        }
        for (int y = 0; y < c.h; ++y) {
            const int lo = p1[sm[kSOffVB] + 2 * y], n = p1[sm[kSOffVB] + 2 * y + 1];
            EXPECT(n >= 1 && n <= sm[kSKsV] && lo >= 0 && lo + n <= sm[kSRows], "sample %d y %d taps [%d, +%d)", s, y, lo, n);
            int64_t sum = 0;
            for (int j = 0; j < n; ++j) sum += p1[sm[kSOffVK] + (int64_t)y * sm[kSKsV] + j];
            EXPECT(std::llabs(sum - (1 << kPrecisionBits)) <= sm[kSKsV], "sample %d y %d coefficients sum to %lld", s, y, (long long)sum);
        }
        std::vector<int> rows_seen((size_t)sm[kSRows], 0), out_seen((size_t)c.h, 0);
        for (int it = 0; it < p1[kHItemsH]; ++it) {
            const int32_t* item = p1 + p1[kHOffItemsH] + 3 * it;
            EXPECT(item[0] >= 0 && item[0] < N, "rows item %d names sample %d", it, item[0]);
            if (item[0] == s)
                for (int r = item[1]; r < item[1] + item[2]; ++r) {
                    EXPECT(r >= 0 && r < sm[kSRows], "rows item %d row %d", it, r);
                    if (r >= 0 && r < sm[kSRows]) ++rows_seen[(size_t)r];
                }
        }
        for (int it = 0; it < p1[kHItemsV]; ++it) {
            const int32_t* item = p1 + p1[kHOffItemsV] + 3 * it;
            EXPECT(item[0] >= 0 && item[0] < N, "bytes item %d names sample %d", it, item[0]);
            if (item[0] == s)
                for (int y = item[1]; y < item[1] + item[2]; ++y) {
                    EXPECT(y >= 0 && y < c.h, "bytes item %d row %d", it, y);
                    if (y >= 0 && y < c.h) ++out_seen[(size_t)y];
                }
        }
        for (int v : rows_seen) EXPECT(v == 1, "sample %d: a scratch row is written %d times", s, v);
        for (int v : out_seen) EXPECT(v == 1, "sample %d: a row of the intermediate is written %d times", s, v);
    }
    EXPECT(mid_next == mid_bytes, "the intermediate is packed: %lld vs %lld", (long long)mid_next, (long long)mid_bytes);
}

// plan + execute a batch of cases, and the same as two single-stage plans one after the other
static void run(const std::vector<Case>& cases, int C, int Ho, int Wo, const std::vector<uint8_t>& flip, uint32_t seed, int gap) {
    const int64_t N = (int64_t)cases.size();
    std::vector<int32_t> geom, geom1, geom2;
    std::vector<int64_t> off, off2;
    int64_t at = gap, mid_total = 0;
    for (const Case& c : cases) {
        geom.insert(geom.end(), {c.H, c.W, c.H1, c.W1, c.y0, c.x0, c.h, c.w});
        geom1.insert(geom1.end(), {c.H, c.W, 0, 0, c.H, c.W, c.H1, c.W1, c.y0, c.x0});
        geom2.insert(geom2.end(), {c.h, c.w, 0, 0, c.h, c.w, Ho, Wo, 0, 0});
        off.push_back(at);
        off2.push_back(mid_total);
        at += (int64_t)c.H * c.W * C + gap;
        mid_total += (int64_t)c.h * c.w * C;
    }
    std::vector<uint8_t> src((size_t)at);      // exactly the bytes the plan is told of: one byte past is a sanitizer report
    for (auto& b : src) b = (uint8_t)(lcg(seed) >> 24);
    ChainLayout L;
    const char* e = chain_layout_of(geom.data(), N, Ho, Wo, L);
    EXPECT(!e, "layout refused: %s", e ? e : "");
    if (e) return;
    std::vector<int32_t> plan((size_t)L.words);      // exactly the words asked for
    e = build_chain_plan(geom.data(), off.data(), N, C, Ho, Wo, at, plan.data(), plan.size() * 4);
    EXPECT(!e, "plan refused: %s", e ? e : "");
    if (e) return;
    EXPECT(!check_chain_header(plan.data(), plan.size() * 4), "header refused: %s", check_chain_header(plan.data(), plan.size() * 4));
    walk(plan, cases, off, C);
    std::vector<int32_t> again((size_t)L.words, -1);
    EXPECT(!build_chain_plan(geom.data(), off.data(), N, C, Ho, Wo, at, again.data(), again.size() * 4) && again == plan, "the plan is not pure");
    std::vector<float> lut((size_t)C * 256);
    for (size_t i = 0; i < lut.size(); ++i) lut[i] = (float)(i % 256);
    std::vector<float> dst((size_t)(N * C * Ho * Wo), -1.0f);
    std::vector<uint8_t> u8((size_t)(N * Ho * Wo * C)), ws((size_t)pair64(plan.data() + kCWsLo), 0xAB);
    execute_chain(src.data(), plan.data(), lut.data(), flip.empty() ? nullptr : flip.data(), dst.data(), u8.data(), ws.data());
    EXPECT(pair64(plan.data() + kCMidLo) == mid_total, "intermediate bytes");
    const uint8_t* mid = ws.data() + pair64(plan.data() + kCMidAtLo);

    // stage 1 alone: each sample's own window of its first resize, as bytes
    std::vector<uint8_t> mid_ref((size_t)mid_total);
    for (int64_t s = 0; s < N; ++s) {
        const Case& c = cases[(size_t)s];
        Layout L1;
        EXPECT(!layout_of(geom1.data() + s * kGeomWords, 1, c.h, c.w, L1), "stage-1 layout");
        std::vector<int32_t> p((size_t)L1.words);
        const int64_t o[1] = {off[(size_t)s]};
        EXPECT(!build_plan(geom1.data() + s * kGeomWords, o, 1, C, c.h, c.w, at, p.data(), p.size() * 4), "stage-1 plan");
        std::vector<float> f((size_t)C * c.h * c.w);
        std::vector<uint8_t> w1((size_t)pair64(p.data() + kHWsLo));
        execute(src.data(), p.data(), lut.data(), nullptr, f.data(), mid_ref.data() + off2[(size_t)s], w1.data());
    }
    EXPECT(std::equal(mid_ref.begin(), mid_ref.end(), mid), "the intermediate differs from the single-stage window");
    // stage 2 alone on that intermediate
    Layout L2;
    EXPECT(!layout_of(geom2.data(), N, Ho, Wo, L2), "stage-2 layout");
    std::vector<int32_t> p2((size_t)L2.words);
    EXPECT(!build_plan(geom2.data(), off2.data(), N, C, Ho, Wo, mid_total, p2.data(), p2.size() * 4), "stage-2 plan");
    std::vector<float> dst_ref(dst.size(), -2.0f);
    std::vector<uint8_t> u8_ref(u8.size()), w2((size_t)pair64(p2.data() + kHWsLo));
    execute(mid_ref.data(), p2.data(), lut.data(), flip.empty() ? nullptr : flip.data(), dst_ref.data(), u8_ref.data(), w2.data());
    EXPECT(u8 == u8_ref && dst == dst_ref, "the chain differs from its two stages run apart");

    // executed from a copy at another address, with another filling of the workspace
    std::vector<int32_t> room(plan.size() + 5);
    std::copy(plan.begin(), plan.end(), room.begin() + 5);
    std::vector<float> dst2(dst.size(), -3.0f);
    std::vector<uint8_t> u82(u8.size()), ws_b(ws.size(), 0x11);
    execute_chain(src.data(), room.data() + 5, lut.data(), flip.empty() ? nullptr : flip.data(), dst2.data(), u82.data(), ws_b.data());
    EXPECT(u82 == u8 && dst2 == dst, "the plan depends on its address or on what the workspace held");
}

static void refusals() {
    std::vector<int32_t> plan(1 << 16);
    const size_t bytes = plan.size() * 4;
    const int64_t off[1] = {0};
    auto refused = [&](std::vector<int32_t> g, int C, int Ho, int Wo, int64_t src_bytes, int64_t o = 0, size_t pb = 0) {
        const int64_t offs[1] = {o};
        plan[kCMagic] = kChainMagic;
        const char* e = build_chain_plan(g.data(), offs, 1, C, Ho, Wo, src_bytes, plan.data(), pb ? pb : bytes);
        return e != nullptr && plan[kCMagic] != kChainMagic;
    };
    const std::vector<int32_t> ok = {8, 6, 12, 9, 1, 1, 5, 4};
    EXPECT(!build_chain_plan(ok.data(), off, 1, 3, 4, 4, 144, plan.data(), bytes), "a valid plan is refused");
    EXPECT(refused({8, 6, 12, 9, 8, 1, 5, 4}, 3, 4, 4, 144), "box past the bottom of H1");
    EXPECT(refused({8, 6, 12, 9, 1, 6, 5, 4}, 3, 4, 4, 144), "box past the right edge of W1");
    EXPECT(refused({8, 6, 12, 9, -1, 0, 5, 4}, 3, 4, 4, 144) && refused({8, 6, 12, 9, 0, -1, 5, 4}, 3, 4, 4, 144), "negative box origin");
    EXPECT(refused({8, 6, 12, 9, 0, 0, 0, 4}, 3, 4, 4, 144) && refused({8, 6, 12, 9, 0, 0, 5, 0}, 3, 4, 4, 144), "empty box");
    EXPECT(refused({8, 6, 0, 9, 0, 0, 5, 4}, 3, 4, 4, 144) && refused({8, 6, 12, -1, 0, 0, 5, 4}, 3, 4, 4, 144), "empty first stage");
    EXPECT(refused({0, 6, 12, 9, 0, 0, 5, 4}, 3, 4, 4, 144) && refused({8, 0, 12, 9, 0, 0, 5, 4}, 3, 4, 4, 144), "empty image");
    EXPECT(refused({16385, 6, 12, 9, 0, 0, 5, 4}, 3, 4, 4, (int64_t)16385 * 6 * 3), "a source side above 16384");
    EXPECT(refused({8, 6, 16385, 9, 0, 0, 5, 4}, 3, 4, 4, 144) && refused({8, 6, 12, 16385, 0, 0, 5, 4}, 3, 4, 4, 144), "a first-stage side above 16384");
    EXPECT(refused({8, 6, 12, 9, 0x7fffffff, 1, 5, 4}, 3, 4, 4, 144), "a box origin that overflows int32 when the side is added");
    EXPECT(refused(ok, 0, 4, 4, 144) && refused(ok, 5, 4, 4, 144), "C outside 1 .. 4");
    EXPECT(refused(ok, 3, 0, 4, 144) && refused(ok, 3, 4, -2, 144) && refused(ok, 3, 16385, 4, 144), "output size");
    EXPECT(refused(ok, 3, 4, 4, 143), "src one byte short");
    EXPECT(refused(ok, 3, 4, 4, 144, 1), "offset + size past src");
    EXPECT(refused(ok, 3, 4, 4, 144, -1), "negative offset");
    EXPECT(refused(ok, 3, 4, 4, -1), "negative src size");
    EXPECT(refused(ok, 3, 4, 4, 144, 0, (size_t)kChainHeaderWords * 4), "plan memory too small");
    EXPECT(build_chain_plan(ok.data(), off, 1, 3, 4, 4, 144, nullptr, bytes) != nullptr, "null plan memory");
    EXPECT(build_chain_plan(ok.data(), off, 1, 3, 4, 4, 144, plan.data(), 8) != nullptr, "short plan memory");
    EXPECT(build_chain_plan(nullptr, off, 1, 3, 4, 4, 144, plan.data(), bytes) != nullptr, "null geometry");
    EXPECT(build_chain_plan(ok.data(), nullptr, 1, 3, 4, 4, 144, plan.data(), bytes) != nullptr, "null offsets");
    EXPECT(build_chain_plan(ok.data(), off, -1, 3, 4, 4, 144, plan.data(), bytes) != nullptr, "negative N");
    // an empty batch is a plan of its own
    EXPECT(!build_chain_plan(nullptr, nullptr, 0, 3, 4, 4, 0, plan.data(), bytes) && plan[kCN] == 0 && !check_chain_header(plan.data(), bytes), "N == 0");
    // headers a launch refuses: the plan handed back short, and every header word of the three parts damaged
    EXPECT(!build_chain_plan(ok.data(), off, 1, 3, 4, 4, 144, plan.data(), bytes), "a valid plan is refused");
    const size_t exact = (size_t)plan[kCWords] * 4;
    EXPECT(!check_chain_header(plan.data(), exact), "the exact size is refused");
    EXPECT(check_chain_header(plan.data(), exact - 4) != nullptr, "plan longer than plan_bytes");
    EXPECT(check_chain_header(nullptr, bytes) != nullptr && check_chain_header(plan.data(), 8) != nullptr, "null or short plan");
    const int off1 = plan[kCOff1], off2 = plan[kCOff2];
    for (int word : {(int)kCMagic, (int)kCN, (int)kCC, (int)kCHo, (int)kCWo, (int)kCWsLo, (int)kCWords, (int)kCOff1, (int)kCOff2, (int)kCMidAtLo,
                     (int)kCMidLo, (int)kCWs2AtLo, off1 + kHMagic, off1 + kHN, off1 + kHC, off1 + kHWsLo, off1 + kHWords, off2 + kHMagic,
                     off2 + kHN, off2 + kHC, off2 + kHHo, off2 + kHWo, off2 + kHSrcLo, off2 + kHWsLo, off2 + kHWords}) {
        for (int32_t flipbit : {1, 1 << 20, (int32_t)0x80000000}) {
            plan[(size_t)word] ^= flipbit;
            EXPECT(check_chain_header(plan.data(), exact) != nullptr, "header word %d ^ %x is accepted", word, (unsigned)flipbit);
            plan[(size_t)word] ^= flipbit;
        }
    }
    EXPECT(!check_chain_header(plan.data(), exact), "the restored plan is refused");
    // a single-stage plan is not a chain plan, nor the reverse
    EXPECT(check_header(plan.data(), bytes) != nullptr, "a chain plan passes for a plan");
    std::vector<int32_t> single(1 << 12);
    const std::vector<int32_t> g10 = {8, 6, 1, 1, 5, 4, 4, 4, 0, 0};
    EXPECT(!build_plan(g10.data(), off, 1, 3, 4, 4, 144, single.data(), single.size() * 4), "a valid single-stage plan is refused");
    EXPECT(check_chain_header(single.data(), single.size() * 4) != nullptr, "a plan passes for a chain plan");
    EXPECT(check_header(plan.data() + off1, exact - 4 * (size_t)off1) != nullptr, "the stage-1 section passes for a plan");
}

int main() {
    struct Named {
        Case c;
        int Ho, Wo;
    };
    const Named named[] = {{{37, 53, 24, 34, 3, 5, 17, 22}, 16, 16}, {{9, 7, 25, 20, 0, 0, 25, 20}, 8, 8},  {{300, 17, 141, 8, 60, 1, 30, 6}, 12, 10},
                           {{24, 40, 24, 40, 2, 3, 20, 30}, 16, 16}, {{1, 1, 4, 4, 0, 0, 4, 4}, 4, 4},      {{20, 31, 12, 18, 11, 17, 1, 1}, 5, 5},
                           {{50, 37, 32, 24, 20, 10, 12, 14}, 7, 9}};
    uint32_t seed = 1;
    std::vector<Case> all;
    for (const Named& n : named) {
        all.push_back(n.c);
        for (int C : {1, 3, 4}) run({n.c}, C, n.Ho, n.Wo, {}, ++seed, 0);
    }
    // all of them as one ragged batch at offsets that are no multiple of 4, flipped and not; the last sample ends where src ends
    for (int C : {1, 2, 3, 4}) {
        run(all, C, 16, 16, {1, 0, 1, 0, 1, 0, 1}, ++seed, 0);
        run(all, C, 7, 9, {}, ++seed, 3);
    }
    // the largest sides the plan admits, and several items per sample in every table
    run({{1, 16384, 1, 16384, 0, 16383, 1, 1}}, 1, 1, 1, {}, ++seed, 0);
    run({{16384, 1, 16384, 2, 16000, 1, 384, 1}}, 2, 3, 2, {1}, ++seed, 1);
    run({{1, 1, 3, 700, 1, 0, 2, 700}}, 4, 1, 700, {}, ++seed, 0);
    run({{310, 290, 280, 262, 10, 5, 260, 250}, {5, 300, 300, 5, 0, 0, 300, 5}}, 3, 224, 224, {0, 1}, ++seed, 1);
    refusals();
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("RESAMPLE_CHAIN_OK\n");
    return 0;
}
