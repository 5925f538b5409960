// Stand-alone check of csrc/rl_query.h, the packed blocks of the pose-query stages (horizon,
// rejoin): byte counts against their closed forms, every byte of the queries' block, the launch
// pointers over a guarded buffer of exactly out_bytes, and the copies into rl_hzn / rl_rjn with
// every field, with alternating fields NULL and from the head alone.  No HIP call; built and run
// by tests/test_query_layout_cpu.py (under AddressSanitizer and UBSan where they link).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rl_query.h"

using namespace rl;

static int g_bad = 0;
#define CHECK(cond, ...)                                             \
    do {                                                             \
        if (!(cond)) {                                               \
            ++g_bad;                                                 \
            std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                                \
            std::printf("\n");                                       \
        }                                                            \
    } while (0)

constexpr size_t GUARD = 64;                 // one cache line on either side
constexpr unsigned char FILL = 0xA5;
enum { A_COL = 0, A_PER = 7, A_INT = 14, A_NODE = 18, A_ALL = 20 };   // array ids: cols, doubles, ints, nodes

static double dval(int a, size_t q, size_t i) { return (double)(a * 100000000LL + (long long)q * 10000 + (long long)i); }
static int32_t ival(int a, size_t q) { return (int32_t)(a * 10000000 + (int)q); }

// a heap buffer of exactly n bytes between two guards
struct Guarded {
    std::vector<unsigned char> mem;
    size_t n;
    explicit Guarded(size_t bytes) : mem(bytes + 2 * GUARD, FILL), n(bytes) {}
    char* data() { return (char*)mem.data() + GUARD; }
    bool intact() const {
        for (size_t i = 0; i < GUARD; ++i)
            if (mem[i] != FILL || mem[GUARD + n + i] != FILL) return false;
        return true;
    }
};

// the destination of one result array: its own exact-size allocation
struct Dest {
    std::vector<double> d;
    std::vector<int32_t> i;
};

static void check_shape(size_t Q, size_t M, size_t K, bool rjn) {
    const size_t Kk = rjn ? K : 0;
    const QueryLayout L = query_layout(Q, M, Kk);
    const char* name = rjn ? "rejoin" : "horizon";
    // ---- byte counts: the closed forms
    const size_t in_want = rjn ? Q * 32 : Q * 24;
    const size_t head_want = rjn ? (7 * Q * M + 7 * Q) * 8 + 4 * Q * 4 : (7 * Q * M + 5 * Q) * 8 + 2 * Q * 4;
    const size_t out_want = rjn ? head_want + 2 * Q * (K + 1) * 8 : head_want;
    CHECK(L.in_bytes == in_want, "%s (%zu,%zu,%zu): in_bytes %zu != %zu", name, Q, M, K, L.in_bytes, in_want);
    CHECK(L.head_bytes == head_want, "%s (%zu,%zu,%zu): head_bytes %zu != %zu", name, Q, M, K, L.head_bytes, head_want);
    CHECK(L.out_bytes == out_want, "%s (%zu,%zu,%zu): out_bytes %zu != %zu", name, Q, M, K, L.out_bytes, out_want);

    // ---- the queries' block, row and seg_hint once given and once NULL
    std::vector<double> pose(2 * Q), v0(Q);
    std::vector<int32_t> row(Q), hint(Q);
    for (size_t k = 0; k < Q; ++k) {
        pose[2 * k] = 1000.5 + (double)k;
        pose[2 * k + 1] = -2000.25 - (double)k;
        v0[k] = 3.125 * (double)(k + 1);
        row[k] = (int32_t)(k + 7);
        hint[k] = (int32_t)(3 * k + 1);
    }
    rl_cfg cfg{};
    Guarded in(L.in_bytes);
    rl_rjn_query q{};
    for (int given = 1; given >= 0; --given) {
        if (rjn)
            q = rl_rjn_query{pose.data(), given ? row.data() : nullptr, given ? hint.data() : nullptr, (int32_t)Q, 3, (int32_t)M, 0,
                             0.05, v0.data(), &cfg, (int32_t)K, 0};
        else
            q = as_rjn(rl_hzn_query{pose.data(), given ? row.data() : nullptr, given ? hint.data() : nullptr, (int32_t)Q, 3,
                                    (int32_t)M, 0, 0.05});
        const QueryLayout Lq = query_layout(q);
        CHECK(Lq.in_bytes == L.in_bytes && Lq.out_bytes == L.out_bytes && Lq.head_bytes == L.head_bytes, "%s: layout of the query", name);
        std::memset(in.data(), FILL, L.in_bytes);
        query_pack(q, L, in.data());
        std::vector<unsigned char> want(in_want);                  // built from the documented order alone
        unsigned char* w = want.data();
        std::memcpy(w, pose.data(), Q * 16); w += Q * 16;
        if (rjn) { std::memcpy(w, v0.data(), Q * 8); w += Q * 8; }
        for (size_t k = 0; k < Q; ++k, w += 4) { const int32_t r = given ? row[k] : 0; std::memcpy(w, &r, 4); }
        for (size_t k = 0; k < Q; ++k, w += 4) { const int32_t g = given ? hint[k] : -1; std::memcpy(w, &g, 4); }
        CHECK(w == want.data() + in_want, "%s: expected block size", name);
        CHECK(std::memcmp(in.data(), want.data(), in_want) == 0, "%s (%zu,%zu,%zu) given=%d: queries' block differs", name, Q, M, K, given);
        CHECK(in.intact(), "%s: guard of the queries' block", name);
    }
    // (in now holds the NULL variant; pack the given one again for the pointer check)
    q.row = row.data();
    q.seg_hint = hint.data();
    query_pack(q, L, in.data());

    // ---- the launch pointers over exactly out_bytes
    Guarded out(L.out_bytes);
    const RjnParams r = query_pointers(q, L, in.data(), out.data());
    const HznParams& h = r.hz;
    CHECK(h.Q == (int32_t)Q && h.M_cap == (int32_t)M && h.window == 3 && h.dt == 0.05, "%s: sizes", name);
    CHECK(r.K_cap == (int32_t)Kk, "%s: K_cap", name);
    for (size_t k = 0; k < Q; ++k) {
        CHECK(h.pose[2 * k] == pose[2 * k] && h.pose[2 * k + 1] == pose[2 * k + 1], "%s: pose[%zu]", name, k);
        CHECK(h.row[k] == row[k] && h.hint[k] == hint[k], "%s: row / hint[%zu]", name, k);
        if (rjn) CHECK(r.v0[k] == v0[k], "%s: v0[%zu]", name, k);
    }
    if (!rjn) CHECK(!r.v0 && !r.scal[0] && !r.scal[1] && !r.merge_node && !r.overspeed && !r.node_v && !r.node_t, "horizon: rejoin pointers");
    double* dptr[A_ALL] = {};
    int32_t* iptr[A_ALL] = {};
    for (int c = 0; c < TRAJ_COLS; ++c) dptr[A_COL + c] = h.out[c];
    for (int c = 0; c < HZN_LOC; ++c) dptr[A_PER + c] = h.loc[c];
    for (int c = 0; c < RJN_SCAL; ++c) dptr[A_PER + HZN_LOC + c] = r.scal[c];
    iptr[A_INT] = h.seg; iptr[A_INT + 1] = h.count; iptr[A_INT + 2] = r.merge_node; iptr[A_INT + 3] = r.overspeed;
    dptr[A_NODE] = r.node_v; dptr[A_NODE + 1] = r.node_t;
    auto width = [&](int a) { return a < A_PER ? M : a < A_NODE ? (size_t)1 : K + 1; };
    auto present = [&](int a) { return rjn || a < A_PER + HZN_LOC || a == A_INT || a == A_INT + 1; };
    for (int a = 0; a < A_ALL; ++a) {
        if (!present(a)) continue;
        CHECK(dptr[a] || iptr[a], "%s: array %d has no pointer", name, a);
        for (size_t k = 0; k < Q; ++k)
            for (size_t i = 0; i < width(a); ++i) {
                if (iptr[a]) iptr[a][k] = ival(a, k);
                else if (dptr[a]) dptr[a][k * width(a) + i] = dval(a, k, i);
            }
    }
    CHECK(out.intact(), "%s (%zu,%zu,%zu): a launch pointer reaches outside out_bytes", name, Q, M, K);

    // ---- the copies out: 0 every field, 1 / 2 alternating fields NULL, 3 (rejoin) no node arrays
    // and only the head to read
    for (int variant = 0; variant < (rjn ? 4 : 3); ++variant) {
        std::vector<char> src(out.data(), out.data() + (variant == 3 ? L.head_bytes : L.out_bytes));   // exact size
        Dest dst[A_ALL];
        bool asked[A_ALL];
        void* f[A_ALL];
        for (int a = 0; a < A_ALL; ++a) {
            const bool ints = a >= A_INT && a < A_NODE;
            if (ints) dst[a].i.assign(Q, -77);
            else dst[a].d.assign(Q * width(a), -77.0);
            asked[a] = present(a) && (variant == 0 || (variant == 3 ? a < A_NODE : a % 2 == variant - 1));
            f[a] = !asked[a] ? nullptr : ints ? (void*)dst[a].i.data() : (void*)dst[a].d.data();
        }
        auto D = [&](int a) { return (double*)f[a]; };
        auto I = [&](int a) { return (int32_t*)f[a]; };
        if (rjn) {
            const rl_rjn o{D(0), D(1), D(2), D(3), D(4), D(5), D(6), D(7), D(8), D(9), D(10), D(11), I(14), I(15),
                           I(16), I(17), D(12), D(13), D(18), D(19)};
            query_unpack(src.data(), L, o);
        } else {
            const rl_hzn o{D(0), D(1), D(2), D(3), D(4), D(5), D(6), D(7), D(8), D(9), D(10), D(11), I(14), I(15)};
            query_unpack(src.data(), L, as_rjn(o));
        }
        for (int a = 0; a < A_ALL; ++a)
            for (size_t k = 0; k < Q; ++k) {
                if (a >= A_INT && a < A_NODE) {
                    const int32_t want = asked[a] ? ival(a, k) : -77;
                    CHECK(dst[a].i[k] == want, "%s (%zu,%zu,%zu) variant %d: array %d [%zu] = %d, not %d", name, Q, M, K, variant, a, k,
                          dst[a].i[k], want);
                    continue;
                }
                for (size_t i = 0; i < width(a); ++i) {
                    const double want = asked[a] ? dval(a, k, i) : -77.0;
                    CHECK(dst[a].d[k * width(a) + i] == want, "%s (%zu,%zu,%zu) variant %d: array %d [%zu][%zu] = %.17g, not %.17g", name,
                          Q, M, K, variant, a, k, i, dst[a].d[k * width(a) + i], want);
                }
            }
    }
    CHECK(out.intact(), "%s: guard of the results' block after the copies", name);
}

int main() {
    const size_t shapes[4][3] = {{1, 1, 1}, {3, 2, 4}, {2, 5, 1024}, {65, 7, 9}};
    for (const auto& s : shapes)
        for (int rjn = 0; rjn < 2; ++rjn) check_shape(s[0], s[1], s[2], rjn != 0);
    if (g_bad) {
        std::printf("query layout: %d checks failed\n", g_bad);
        return 1;
    }
    std::printf("query layout ok: 4 shapes x (horizon, rejoin)\n");
    return 0;
}
