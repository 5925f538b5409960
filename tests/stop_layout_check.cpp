// Stand-alone check of the stop stage's packed blocks in csrc/rl_query.h: byte counts against
// their closed forms, every offset of a rejoin layout unchanged beside it, every byte of the
// queries' block (v_target given and NULL), the launch pointers over a guarded buffer of exactly
// out_bytes, and the copies into rl_stp with every field, with alternating fields NULL and from
// the head alone.  No HIP call; built and run by tests/test_stop_layout_cpu.py (under
// AddressSanitizer and UBSan where they link).
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
// array ids in rl_stp's order of kinds: 7 columns, 9 doubles [Q], 6 ints [Q], 3 node arrays
enum { A_COL = 0, A_PER = 7, A_INT = 16, A_NODE = 22, A_ALL = 25 };

static double dval(int a, size_t q, size_t i) { return (double)(a * 100000000LL + (long long)q * 10000 + (long long)i); }
static int32_t ival(int a, size_t q) { return (int32_t)(a * 10000000 + (int)q); }

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

static void check_shape(size_t Q, size_t M, size_t K) {
    const QueryLayout L = query_layout(Q, M, K, true);
    const QueryLayout R = query_layout(Q, M, K);                   // the rejoin layout of the same sizes
    // ---- byte counts: the closed forms
    const size_t in_want = Q * 44;
    const size_t head_want = (7 * Q * M + 9 * Q) * 8 + 6 * Q * 4;
    const size_t out_want = head_want + 3 * Q * (K + 1) * 8;
    CHECK(L.in_bytes == in_want, "(%zu,%zu,%zu): in_bytes %zu != %zu", Q, M, K, L.in_bytes, in_want);
    CHECK(L.head_bytes == head_want, "(%zu,%zu,%zu): head_bytes %zu != %zu", Q, M, K, L.head_bytes, head_want);
    CHECK(L.out_bytes == out_want, "(%zu,%zu,%zu): out_bytes %zu != %zu", Q, M, K, L.out_bytes, out_want);
    CHECK(L.stop && !R.stop && R.in_bytes == Q * 32, "the rejoin layout has no stop arrays");
    // the rejoin part of the queries' block lies where the rejoin stage has it; every array is aligned
    CHECK(L.pose == R.pose && L.v0 == R.v0 && L.row == R.row && L.hint == R.hint && L.v_target == R.in_bytes, "queries' block");
    CHECK(L.v_target % 8 == 0 && L.stop_sample % 4 == 0 && L.node_b % 8 == 0 && L.nodes[0] % 8 == 0, "alignment");
    for (size_t o : L.sper) CHECK(o % 8 == 0, "alignment of a double array");

    // ---- the queries' block, v_target once given and once NULL
    std::vector<double> pose(2 * Q), v0(Q), vt(Q);
    std::vector<int32_t> row(Q), hint(Q), js(Q);
    for (size_t k = 0; k < Q; ++k) {
        pose[2 * k] = 1000.5 + (double)k;
        pose[2 * k + 1] = -2000.25 - (double)k;
        v0[k] = 3.125 * (double)(k + 1);
        vt[k] = 0.5 * (double)(k + 3);
        row[k] = (int32_t)(k + 7);
        hint[k] = (int32_t)(3 * k + 1);
        js[k] = (int32_t)(5 * k + 2);
    }
    rl_cfg cfg{};
    Guarded in(L.in_bytes);
    rl_stp_query q{};
    for (int given = 1; given >= 0; --given) {
        q = rl_stp_query{rl_rjn_query{pose.data(), row.data(), hint.data(), (int32_t)Q, 3, (int32_t)M, 0, 0.05, v0.data(), &cfg,
                                      (int32_t)K, 0},
                         js.data(), given ? vt.data() : nullptr};
        const QueryLayout Lq = query_layout(q);
        CHECK(Lq.stop && Lq.in_bytes == L.in_bytes && Lq.out_bytes == L.out_bytes && Lq.head_bytes == L.head_bytes, "layout of the query");
        std::memset(in.data(), FILL, L.in_bytes);
        query_pack(q, L, in.data());
        std::vector<unsigned char> want(in_want);                  // built from the documented order alone
        unsigned char* w = want.data();
        std::memcpy(w, pose.data(), Q * 16); w += Q * 16;
        std::memcpy(w, v0.data(), Q * 8); w += Q * 8;
        std::memcpy(w, row.data(), Q * 4); w += Q * 4;
        std::memcpy(w, hint.data(), Q * 4); w += Q * 4;
        for (size_t k = 0; k < Q; ++k, w += 8) { const double t = given ? vt[k] : 0.0; std::memcpy(w, &t, 8); }
        std::memcpy(w, js.data(), Q * 4); w += Q * 4;
        CHECK(w == want.data() + in_want, "expected block size");
        CHECK(std::memcmp(in.data(), want.data(), in_want) == 0, "(%zu,%zu,%zu) given=%d: queries' block differs", Q, M, K, given);
        CHECK(in.intact(), "guard of the queries' block");
    }
    // a query without a stop_sample is a rejoin query, laid out as one
    const rl_stp_query plain = as_stp(q.rj);
    CHECK(!query_layout(plain).stop && query_layout(plain).out_bytes == R.out_bytes, "as_stp of a rejoin query");
    q.v_target = vt.data();
    query_pack(q, L, in.data());

    // ---- the launch pointers over exactly out_bytes
    Guarded out(L.out_bytes);
    const StpParams s = query_pointers(q, L, in.data(), out.data());
    const RjnParams& r = s.rj;
    const HznParams& h = r.hz;
    CHECK(h.Q == (int32_t)Q && h.M_cap == (int32_t)M && h.window == 3 && h.dt == 0.05 && r.K_cap == (int32_t)K, "sizes");
    for (size_t k = 0; k < Q; ++k) {
        CHECK(h.pose[2 * k] == pose[2 * k] && h.pose[2 * k + 1] == pose[2 * k + 1], "pose[%zu]", k);
        CHECK(h.row[k] == row[k] && h.hint[k] == hint[k] && r.v0[k] == v0[k], "row / hint / v0[%zu]", k);
        CHECK(s.v_target[k] == vt[k] && s.stop_sample[k] == js[k], "v_target / stop_sample[%zu]", k);
    }
    const StpParams none = query_pointers(plain, R, in.data(), out.data());
    CHECK(!none.v_target && !none.stop_sample && !none.reachable && !none.brake_node && !none.scal[0] && !none.scal[1] && !none.node_b,
          "rejoin: stop pointers");
    double* dptr[A_ALL] = {};
    int32_t* iptr[A_ALL] = {};
    for (int c = 0; c < TRAJ_COLS; ++c) dptr[A_COL + c] = h.out[c];
    for (int c = 0; c < HZN_LOC; ++c) dptr[A_PER + c] = h.loc[c];
    for (int c = 0; c < RJN_SCAL; ++c) dptr[A_PER + HZN_LOC + c] = r.scal[c];
    for (int c = 0; c < STP_SCAL; ++c) dptr[A_PER + HZN_LOC + RJN_SCAL + c] = s.scal[c];
    iptr[A_INT] = h.seg; iptr[A_INT + 1] = h.count; iptr[A_INT + 2] = r.merge_node; iptr[A_INT + 3] = r.overspeed;
    iptr[A_INT + 4] = s.reachable; iptr[A_INT + 5] = s.brake_node;
    dptr[A_NODE] = r.node_v; dptr[A_NODE + 1] = r.node_t; dptr[A_NODE + 2] = s.node_b;
    auto width = [&](int a) { return a < A_PER ? M : a < A_NODE ? (size_t)1 : K + 1; };
    for (int a = 0; a < A_ALL; ++a) {
        CHECK(dptr[a] || iptr[a], "array %d has no pointer", a);
        for (size_t k = 0; k < Q; ++k)
            for (size_t i = 0; i < width(a); ++i) {
                if (iptr[a]) iptr[a][k] = ival(a, k);
                else if (dptr[a]) dptr[a][k * width(a) + i] = dval(a, k, i);
            }
    }
    CHECK(out.intact(), "(%zu,%zu,%zu): a launch pointer reaches outside out_bytes", Q, M, K);
    // every head array lies before head_bytes, every node array behind it
    for (int a = 0; a < A_ALL; ++a) {
        const char* at = iptr[a] ? (const char*)iptr[a] : (const char*)dptr[a];
        const size_t off = (size_t)(at - out.data());
        CHECK(a < A_NODE ? off < L.head_bytes : off >= L.head_bytes, "array %d on the wrong side of the head", a);
    }

    // ---- the copies out: 0 every field, 1 / 2 alternating fields NULL, 3 no node arrays and only
    // the head to read, 4 node_b alone of the node arrays
    for (int variant = 0; variant < 5; ++variant) {
        std::vector<char> src(out.data(), out.data() + (variant == 3 ? L.head_bytes : L.out_bytes));   // exact size
        std::vector<double> dd[A_ALL];
        std::vector<int32_t> di[A_ALL];
        bool asked[A_ALL];
        void* f[A_ALL];
        for (int a = 0; a < A_ALL; ++a) {
            const bool ints = a >= A_INT && a < A_NODE;
            if (ints) di[a].assign(Q, -77);
            else dd[a].assign(Q * width(a), -77.0);
            asked[a] = variant == 0 || (variant == 3 ? a < A_NODE : variant == 4 ? a == A_NODE + 2 : a % 2 == variant - 1);
            f[a] = !asked[a] ? nullptr : ints ? (void*)di[a].data() : (void*)dd[a].data();
        }
        auto D = [&](int a) { return (double*)f[a]; };
        auto I = [&](int a) { return (int32_t*)f[a]; };
        const rl_stp o{D(0), D(1), D(2), D(3), D(4), D(5), D(6), D(7), D(8), D(9), D(10), D(11), I(16), I(17),
                       I(18), I(19), D(12), D(13), D(22), D(23), I(20), I(21), D(14), D(15), D(24)};
        CHECK(query_wants_nodes(o) == (variant != 3), "variant %d: query_wants_nodes", variant);
        query_unpack(src.data(), L, o);
        for (int a = 0; a < A_ALL; ++a)
            for (size_t k = 0; k < Q; ++k) {
                if (a >= A_INT && a < A_NODE) {
                    const int32_t want = asked[a] ? ival(a, k) : -77;
                    CHECK(di[a][k] == want, "(%zu,%zu,%zu) variant %d: array %d [%zu] = %d, not %d", Q, M, K, variant, a, k, di[a][k], want);
                    continue;
                }
                for (size_t i = 0; i < width(a); ++i) {
                    const double want = asked[a] ? dval(a, k, i) : -77.0;
                    CHECK(dd[a][k * width(a) + i] == want, "(%zu,%zu,%zu) variant %d: array %d [%zu][%zu] = %.17g, not %.17g", Q, M, K,
                          variant, a, k, i, dd[a][k * width(a) + i], want);
                }
            }
    }
    CHECK(out.intact(), "guard of the results' block after the copies");
}

int main() {
    const size_t shapes[4][3] = {{1, 1, 1}, {3, 2, 4}, {2, 5, 1024}, {65, 7, 9}};
    for (const auto& s : shapes) check_shape(s[0], s[1], s[2]);
    if (g_bad) {
        std::printf("stop layout: %d checks failed\n", g_bad);
        return 1;
    }
    std::printf("stop layout ok: 4 shapes\n");
    return 0;
}
