// Stand-alone check of the recover stage's packed blocks in csrc/rl_query.h: byte counts against
// their closed forms, every offset of a retime layout unchanged beside it, the queries' block (the
// rejoin stage's, then merge_len and dir, also with dir_xy NULL), every launch pointer 8-byte
// aligned (4 for the ints) over a guarded buffer of exactly out_bytes, and the copies into rl_rcv
// with every field, with alternating fields NULL and from the head alone.  No HIP call; built and
// run by tests/test_recover_cpu.py (under AddressSanitizer and UBSan where they link).
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

constexpr size_t GUARD = 64;
constexpr unsigned char FILL = 0xA5;
// array ids in kinds: 8 columns (offset last), 10 doubles [Q], 9 ints [Q], 6 node arrays
enum { A_COL = 0, A_PER = 8, A_INT = 18, A_NODE = 27, A_ALL = 33 };

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
    const QueryLayout L = recover_layout(Q, M, K);
    const QueryLayout T = query_layout(Q, M, K, false, true);      // the retime layout of the same sizes
    // ---- byte counts: the closed forms (the ints' pad keeps the node arrays 8-byte aligned)
    const size_t head_want = (8 * Q * M + 10 * Q) * 8 + 10 * Q * 4;
    const size_t out_want = head_want + 6 * Q * (K + 1) * 8;
    CHECK(L.in_bytes == Q * 56 && T.in_bytes == Q * 32, "(%zu,%zu,%zu): in_bytes %zu", Q, M, K, L.in_bytes);
    CHECK(L.head_bytes == head_want, "(%zu,%zu,%zu): head_bytes %zu != %zu", Q, M, K, L.head_bytes, head_want);
    CHECK(L.out_bytes == out_want, "(%zu,%zu,%zu): out_bytes %zu != %zu", Q, M, K, L.out_bytes, out_want);
    CHECK(L.recover && L.retime && !L.stop && !T.recover && T.retime, "flags");
    CHECK(L.pose == T.pose && L.v0 == T.v0 && L.row == T.row && L.hint == T.hint, "the rejoin part of the queries' block");
    CHECK(L.merge_len == T.in_bytes && L.dir == L.merge_len + Q * 8 && L.merge_len % 8 == 0, "merge_len and dir lie behind hint");
    // without the flag nothing moves: the retime layout is what it was
    CHECK(T.head_bytes == (7 * Q * M + 8 * Q) * 8 + 6 * Q * 4 && T.out_bytes == T.head_bytes + 4 * Q * (K + 1) * 8, "retime layout: closed forms");
    CHECK(query_layout(Q, M, K).out_bytes == (7 * Q * M + 7 * Q) * 8 + 4 * Q * 4 + 2 * Q * (K + 1) * 8, "rejoin layout: closed form");
    for (int c = 0; c < TRAJ_COLS; ++c) CHECK(L.col[c] == T.col[c], "column %d moved", c);
    CHECK(L.offset == 7 * Q * M * 8, "offset lies behind the seven columns");
    CHECK(L.nodes[0] == L.head_bytes && L.cnodes[1] + Q * (K + 1) * 8 == L.out_bytes, "node arrays");

    // ---- the queries' block
    std::vector<double> pose(2 * Q), v0(Q), len(Q), dir(2 * Q);
    std::vector<int32_t> row(Q), hint(Q);
    for (size_t k = 0; k < Q; ++k) {
        pose[2 * k] = 1000.5 + (double)k;
        pose[2 * k + 1] = -2000.25 - (double)k;
        v0[k] = 3.125 * (double)(k + 1);
        len[k] = 10.5 + (double)k;
        dir[2 * k] = 0.25 * (double)(k + 1);
        dir[2 * k + 1] = -0.5 * (double)(k + 1);
        row[k] = (int32_t)(k + 7);
        hint[k] = (int32_t)(3 * k + 1);
    }
    rl_cfg cfg{};
    cfg.v_cap_mps = 27.5; cfg.a_lat_max = 9.25; cfg.kappa_eps = 1e-6;
    const double* const bnd[4] = {pose.data(), v0.data(), len.data(), dir.data()};   // (four distinct addresses)
    for (int with_dir = 1; with_dir >= 0; --with_dir) {
        const rl_rcv_query cq{rl_rjn_query{pose.data(), row.data(), hint.data(), (int32_t)Q, 3, (int32_t)M, 0, 0.05, v0.data(), &cfg,
                                           (int32_t)K, 0},
                              len.data(), with_dir ? dir.data() : nullptr};
        const rl_stp_query q = as_stp(cq.rj);
        const QueryLayout Lq = recover_layout(cq);
        CHECK(Lq.recover && Lq.in_bytes == L.in_bytes && Lq.out_bytes == L.out_bytes && Lq.head_bytes == L.head_bytes, "layout of the query");
        Guarded in(L.in_bytes), in_t(T.in_bytes);
        query_pack(q, L, in.data());
        recover_pack(cq, L, in.data());
        query_pack(q, T, in_t.data());
        CHECK(std::memcmp(in.data(), in_t.data(), T.in_bytes) == 0, "the rejoin part differs from the retime stage's block");
        CHECK(std::memcmp(in.data() + L.merge_len, len.data(), Q * 8) == 0, "merge_len");
        if (with_dir) CHECK(std::memcmp(in.data() + L.dir, dir.data(), Q * 16) == 0, "dir");
        CHECK(in.intact() && in_t.intact(), "guard of the queries' block");

        // ---- the launch pointers over exactly out_bytes
        Guarded out(L.out_bytes);
        const StpParams s = query_pointers(q, L, in.data(), out.data());
        const RcvParams c = recover_pointers(retime_pointers(s.rj, cfg, L, out.data()), cq, L, in.data(), out.data(), bnd);
        const RtmParams& t = c.rt;
        const RjnParams& r = t.rj;
        const HznParams& h = r.hz;
        CHECK(h.Q == (int32_t)Q && h.M_cap == (int32_t)M && r.K_cap == (int32_t)K && t.v_cap == 27.5, "sizes and cfg");
        CHECK(c.lo == bnd[0] && c.hi == bnd[1] && c.nx == bnd[2] && c.ny == bnd[3], "the bounds rows");
        CHECK((c.dir != nullptr) == (with_dir != 0), "a NULL dir_xy gives a null dir");
        for (size_t k = 0; k < Q; ++k) {
            CHECK(c.merge_len[k] == len[k] && r.v0[k] == v0[k] && h.row[k] == row[k], "merge_len / v0 / row[%zu]", k);
            if (with_dir) CHECK(c.dir[2 * k] == dir[2 * k] && c.dir[2 * k + 1] == dir[2 * k + 1], "dir[%zu]", k);
        }
        double* dptr[A_ALL] = {};
        int32_t* iptr[A_ALL] = {};
        for (int i = 0; i < TRAJ_COLS; ++i) dptr[A_COL + i] = h.out[i];
        dptr[A_COL + 7] = c.offset;
        for (int i = 0; i < HZN_LOC; ++i) dptr[A_PER + i] = h.loc[i];
        dptr[A_PER + 5] = r.scal[0]; dptr[A_PER + 6] = r.scal[1]; dptr[A_PER + 7] = t.v_excess;
        dptr[A_PER + 8] = c.scal[0]; dptr[A_PER + 9] = c.scal[1];
        iptr[A_INT] = h.seg; iptr[A_INT + 1] = h.count; iptr[A_INT + 2] = r.merge_node; iptr[A_INT + 3] = r.overspeed;
        iptr[A_INT + 4] = t.feasible; iptr[A_INT + 5] = t.bind_node;
        iptr[A_INT + 6] = c.clamped; iptr[A_INT + 7] = c.offtrack; iptr[A_INT + 8] = c.merge_node;
        dptr[A_NODE] = r.node_v; dptr[A_NODE + 1] = r.node_t; dptr[A_NODE + 2] = t.node_b; dptr[A_NODE + 3] = t.node_c;
        dptr[A_NODE + 4] = c.node_o; dptr[A_NODE + 5] = c.node_k;
        auto width = [&](int a) { return a < A_PER ? M : a < A_NODE ? (size_t)1 : K + 1; };
        for (int a = 0; a < A_ALL; ++a) {
            CHECK(dptr[a] || iptr[a], "array %d has no pointer", a);
            const char* at = iptr[a] ? (const char*)iptr[a] : (const char*)dptr[a];
            const size_t off = (size_t)(at - out.data());
            CHECK(off % (iptr[a] ? 4 : 8) == 0, "(%zu,%zu,%zu): array %d at %zu is misaligned", Q, M, K, a, off);
            CHECK(a < A_NODE ? off < L.head_bytes : off >= L.head_bytes, "array %d on the wrong side of the head", a);
            for (size_t k = 0; k < Q; ++k)
                for (size_t i = 0; i < width(a); ++i) {
                    if (iptr[a]) iptr[a][k] = ival(a, k);
                    else if (dptr[a]) dptr[a][k * width(a) + i] = dval(a, k, i);
                }
        }
        CHECK(out.intact(), "(%zu,%zu,%zu): a launch pointer reaches outside out_bytes", Q, M, K);

        // ---- the copies out: 0 every field, 1 / 2 alternating fields NULL, 3 no node arrays and
        // only the head to read, 4 node_k alone of the node arrays
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
                asked[a] = variant == 0 || (variant == 3 ? a < A_NODE : variant == 4 ? a == A_NODE + 5 : a % 2 == variant - 1);
                f[a] = !asked[a] ? nullptr : ints ? (void*)di[a].data() : (void*)dd[a].data();
            }
            auto D = [&](int a) { return (double*)f[a]; };
            auto I = [&](int a) { return (int32_t*)f[a]; };
            const rl_rcv o{D(0), D(1), D(2), D(3), D(4), D(5), D(6), D(8), D(9), D(10), D(11), D(12), I(18), I(19),
                           I(20), I(21), D(13), D(14), D(27), D(28), I(22), I(23), D(15), D(29), D(30),
                           D(7), I(24), I(25), I(26), D(16), D(17), D(31), D(32)};
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
                        CHECK(dd[a][k * width(a) + i] == want, "(%zu,%zu,%zu) variant %d: array %d [%zu][%zu] = %.17g, not %.17g", Q, M,
                              K, variant, a, k, i, dd[a][k * width(a) + i], want);
                    }
                }
        }
        CHECK(out.intact(), "guard of the results' block after the copies");
    }
}

int main() {
    const size_t shapes[5][3] = {{1, 1, 1}, {3, 2, 4}, {2, 5, 512}, {65, 7, 9}, {70, 64, 16}};
    for (const auto& s : shapes) check_shape(s[0], s[1], s[2]);
    if (g_bad) {
        std::printf("recover layout: %d checks failed\n", g_bad);
        return 1;
    }
    std::printf("recover layout ok: 5 shapes\n");
    return 0;
}
