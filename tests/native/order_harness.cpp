// The dispatch-order logic of the K1 march (csrc/k1_order.h) on the CPU under AddressSanitizer + UBSan: random records of
// many sizes and class counts, in heap buffers of exactly `words` words, so a read or write outside the tables is an error.
// Every table is checked against a sort-based restatement: a permutation inside each XCD's slots, classes descending,
// slot order inside a class, the identity for a zero record.  Plain C++, no HIP, host code only; built and run by
// tests/test_k1_order_host.py::test_header_under_sanitizers.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "k1_order.h"

using namespace mrirt;

static int g_failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_failures <= 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)(g_rng >> 16); }

// the definition, by sorting: threshold j = the value of rank j * n / C; class = thresholds reached
static void check_table(const uint32_t* steps, const uint32_t* order, uint32_t words, uint32_t classes, const char* what) {
    const uint32_t C = classes == 0 ? kOrderDefaultClasses : std::min(classes, kOrderMaxClasses);
    std::vector<uint8_t> seen(words, 0);
    for (uint32_t xcd = 0; xcd < kOrderXcds; ++xcd) {
        std::vector<uint32_t> v;
        for (uint32_t b = xcd; b < words; b += kOrderXcds) v.push_back(steps[b]);
        const uint32_t n = (uint32_t)v.size();
        CHECK(n == order_slots(words, xcd), "%s: order_slots(%u, %u) = %u, counted %u", what, words, xcd, order_slots(words, xcd), n);
        if (n == 0) continue;
        std::vector<uint32_t> sorted(v);
        std::sort(sorted.begin(), sorted.end());
        std::vector<uint32_t> thr;
        for (uint32_t j = 1; j < C; ++j) thr.push_back(sorted[(size_t)(((uint64_t)j * n) / C)]);
        auto cls = [&](uint32_t x) { uint32_t c = 0; for (uint32_t t : thr) c += x >= t ? 1u : 0u; return c; };
        const bool zero = sorted.back() == 0;
        uint32_t prevClass = C, prevSlot = 0;
        for (uint32_t pos = 0; pos < n; ++pos) {
            const uint32_t e = order[pos * kOrderXcds + xcd];
            CHECK(e < words && e % kOrderXcds == xcd, "%s: entry %u of XCD %u is %u (words %u)", what, pos, xcd, e, words);
            if (e >= words || e % kOrderXcds != xcd) continue;
            CHECK(seen[e] == 0, "%s: position %u twice", what, e);
            seen[e] = 1;
            const uint32_t k = e / kOrderXcds, c = cls(v[k]);
            if (zero) CHECK(k == pos, "%s: zero record, XCD %u entry %u is slot %u", what, xcd, pos, k);
            CHECK(c <= prevClass, "%s: XCD %u entry %u: class %u after class %u", what, xcd, pos, c, prevClass);
            if (c == prevClass) CHECK(k > prevSlot, "%s: XCD %u entry %u: slot %u after slot %u in class %u", what, xcd, pos, k, prevSlot, c);
            prevClass = c; prevSlot = k;
        }
    }
    for (uint32_t b = 0; b < words; ++b) CHECK(seen[b] == 1, "%s: position %u never marched", what, b);
}

int main() {
    const uint32_t sizes[] = { 0, 1, 5, 7, 8, 9, 13, 63, 64, 100, 511, 512, 1031, 4096, 4104 };
    const uint32_t classCounts[] = { 0, 1, 2, 3, 4, 8, 16, 40 };
    int cases = 0;
    for (uint32_t words : sizes)
        for (uint32_t classes : classCounts)
            for (int dist = 0; dist < 6; ++dist) {
                // exactly `words` words each (new uint32_t[0] is a valid zero-length buffer ASan still guards)
                uint32_t* steps = new uint32_t[words];
                uint32_t* order = new uint32_t[words];
                for (uint32_t b = 0; b < words; ++b) {
                    const uint32_t r = rnd();
                    steps[b] = dist == 0 ? 0u : dist == 1 ? r % 700u : dist == 2 ? r % 3u : dist == 3 ? (r % 4u == 0 ? r % 1000u : 0u)
                             : dist == 4 ? r : 0xFFFFFFFFu - r % 5u;
                    order[b] = 0xDEADBEEFu;
                }
                order_build_table(steps, words, classes, order);
                char what[96];
                std::snprintf(what, sizeof what, "words %u classes %u dist %d", words, classes, dist);
                check_table(steps, order, words, classes, what);
                delete[] steps;
                delete[] order;
                ++cases;
            }
    if (g_failures != 0) { std::printf("order_harness: %d failures\n", g_failures); return 1; }
    std::printf("order_harness: %d cases ok\n", cases);
    return 0;
}
