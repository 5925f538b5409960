// Stand-alone check of the retime stage's packed blocks in csrc/rl_query.h: byte counts against
// their closed forms, every offset of a rejoin layout unchanged beside it (and of a stop layout
// with and without the flag), the queries' block equal to the rejoin stage's byte for byte, the
// launch pointers over a guarded buffer of exactly out_bytes, and the copies into rl_rtm with every
// field, with alternating fields NULL and from the head alone.  No HIP call; built and run by
// tests/test_retime_cpu.py (under AddressSanitizer and UBSan where they link).
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
// array ids in rl_rtm's order of kinds: 7 columns, 8 doubles [Q], 6 ints [Q], 4 node arrays
enum { A_COL = 0, A_PER = 7, A_INT = 15, A_NODE = 21, A_ALL = 25 };

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
    const QueryLayout L = query_layout(Q, M, K, false, true);
    const QueryLayout R = query_layout(Q, M, K);                   // the rejoin layout of the same sizes
    // ---- byte counts: the closed forms
    const size_t head_want = (7 * Q * M + 8 * Q) * 8 + 6 * Q * 4;
    const size_t out_want = head_want + 4 * Q * (K + 1) * 8;
    CHECK(L.in_bytes == Q * 32 && L.in_bytes == R.in_bytes, "(%zu,%zu,%zu): in_bytes %zu", Q, M, K, L.in_bytes);
    CHECK(L.head_bytes == head_want, "(%zu,%zu,%zu): head_bytes %zu != %zu", Q, M, K, L.head_bytes, head_want);
    CHECK(L.out_bytes == out_want, "(%zu,%zu,%zu): out_bytes %zu != %zu", Q, M, K, L.out_bytes, out_want);
    CHECK(L.retime && !L.stop && !R.retime && !R.stop, "flags");
    CHECK(L.pose == R.pose && L.v0 == R.v0 && L.row == R.row && L.hint == R.hint, "queries' block");
    // without the flag nothing moves: the default arguments give the layouts of before, and the
    // retime arrays take no room in them
    const QueryLayout S1 = query_layout(Q, M, K, true), S0 = query_layout(Q, M, K, true, false);
    CHECK(S1.in_bytes == S0.in_bytes && S1.head_bytes == S0.head_bytes && S1.out_bytes == S0.out_bytes && S1.node_b == S0.node_b,
          "stop layout");
    CHECK(S1.head_bytes == (7 * Q * M + 9 * Q) * 8 + 6 * Q * 4 && S1.out_bytes == S1.head_bytes + 3 * Q * (K + 1) * 8, "stop layout: closed forms");
    CHECK(R.head_bytes == (7 * Q * M + 7 * Q) * 8 + 4 * Q * 4 && R.out_bytes == R.head_bytes + 2 * Q * (K + 1) * 8, "rejoin layout: closed forms");
    for (int c = 0; c < TRAJ_COLS; ++c) CHECK(L.col[c] == R.col[c], "column %d moved", c);
    for (int c = 0; c < QRY_PER; ++c) CHECK(L.per[c] == R.per[c], "double array %d moved", c);
    CHECK(L.rper[0] == R.per[QRY_PER - 1] + Q * 8 && L.rper[0] % 8 == 0, "v_excess lies behind the rejoin stage's doubles");
    CHECK(L.rints[0] % 4 == 0 && L.rints[1] == L.rints[0] + Q * 4 && L.rints[1] + Q * 4 == L.head_bytes, "the ints end the head");
    CHECK(L.nodes[0] == L.head_bytes && L.rnodes[0] == L.nodes[1] + Q * (K + 1) * 8 && L.rnodes[1] + Q * (K + 1) * 8 == L.out_bytes,
          "node arrays");
    CHECK(L.nodes[0] % 8 == 0 && L.rnodes[0] % 8 == 0 && L.rnodes[1] % 8 == 0, "alignment");

    // ---- the queries' block: the rejoin stage's, byte for byte
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
    cfg.v_cap_mps = 27.5; cfg.a_lat_max = 9.25; cfg.kappa_eps = 1e-6;
    const rl_rtm_query tq{rl_rjn_query{pose.data(), row.data(), hint.data(), (int32_t)Q, 3, (int32_t)M, 0, 0.05, v0.data(), &cfg,
                                       (int32_t)K, 0}};
    const rl_stp_query q = as_stp(tq.rj);
    const QueryLayout Lq = query_layout(q, true);
    CHECK(Lq.retime && !Lq.stop && Lq.in_bytes == L.in_bytes && Lq.out_bytes == L.out_bytes && Lq.head_bytes == L.head_bytes, "layout of the query");
    CHECK(!query_layout(q).retime && query_layout(q).out_bytes == R.out_bytes, "a rejoin query without the flag");
    Guarded in(L.in_bytes), in_r(R.in_bytes);
    query_pack(q, L, in.data());
    query_pack(q, R, in_r.data());
    CHECK(std::memcmp(in.data(), in_r.data(), L.in_bytes) == 0, "(%zu,%zu,%zu): queries' block differs from the rejoin stage's", Q, M, K);
    CHECK(in.intact() && in_r.intact(), "guard of the queries' block");

    // ---- the launch pointers over exactly out_bytes
    Guarded out(L.out_bytes);
    const StpParams s = query_pointers(q, L, in.data(), out.data());
    CHECK(!s.v_target && !s.stop_sample && !s.reachable && !s.brake_node && !s.scal[0] && !s.scal[1] && !s.node_b, "stop pointers");
    const RtmParams t = retime_pointers(s.rj, cfg, L, out.data());
    const RjnParams& r = t.rj;
    const HznParams& h = r.hz;
    CHECK(h.Q == (int32_t)Q && h.M_cap == (int32_t)M && h.window == 3 && h.dt == 0.05 && r.K_cap == (int32_t)K, "sizes");
    CHECK(t.v_cap == 27.5 && t.a_lat_max == 9.25 && t.kappa_eps == 1e-6, "the ceiling's cfg fields");
    for (size_t k = 0; k < Q; ++k) {
        CHECK(h.pose[2 * k] == pose[2 * k] && h.pose[2 * k + 1] == pose[2 * k + 1], "pose[%zu]", k);
        CHECK(h.row[k] == row[k] && h.hint[k] == hint[k] && r.v0[k] == v0[k], "row / hint / v0[%zu]", k);
    }
    double* dptr[A_ALL] = {};
    int32_t* iptr[A_ALL] = {};
    for (int c = 0; c < TRAJ_COLS; ++c) dptr[A_COL + c] = h.out[c];
    for (int c = 0; c < HZN_LOC; ++c) dptr[A_PER + c] = h.loc[c];
    for (int c = 0; c < RJN_SCAL; ++c) dptr[A_PER + HZN_LOC + c] = r.scal[c];
    dptr[A_PER + HZN_LOC + RJN_SCAL] = t.v_excess;
    iptr[A_INT] = h.seg; iptr[A_INT + 1] = h.count; iptr[A_INT + 2] = r.merge_node; iptr[A_INT + 3] = r.overspeed;
    iptr[A_INT + 4] = t.feasible; iptr[A_INT + 5] = t.bind_node;
    dptr[A_NODE] = r.node_v; dptr[A_NODE + 1] = r.node_t; dptr[A_NODE + 2] = t.node_b; dptr[A_NODE + 3] = t.node_c;
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
    // the head to read, 4 node_c alone of the node arrays
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
            asked[a] = variant == 0 || (variant == 3 ? a < A_NODE : variant == 4 ? a == A_NODE + 3 : a % 2 == variant - 1);
            f[a] = !asked[a] ? nullptr : ints ? (void*)di[a].data() : (void*)dd[a].data();
        }
        auto D = [&](int a) { return (double*)f[a]; };
        auto I = [&](int a) { return (int32_t*)f[a]; };
        const rl_rtm o{D(0), D(1), D(2), D(3), D(4), D(5), D(6), D(7), D(8), D(9), D(10), D(11), I(15), I(16),
                       I(17), I(18), D(12), D(13), D(21), D(22), I(19), I(20), D(14), D(23), D(24)};
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
        std::printf("retime layout: %d checks failed\n", g_bad);
        return 1;
    }
    std::printf("retime layout ok: 4 shapes\n");
    return 0;
}
