// Stand-alone check of the fan stage's packed blocks in csrc/rl_query.h: byte counts against their
// closed forms, every offset of a recover layout unchanged beside it, the queries' block with
// merge_len [Q][C], every launch pointer of the results' and of the scratch block aligned and
// disjoint over guarded buffers of exactly out_bytes and scratch_bytes, the candidates' launch on
// the query's own pointers, and the copies into rl_fan with every field, without the node arrays
// (from the head alone) and with the table alone.  No HIP call; built and run by
// tests/test_recover_fan_cpu.py (under AddressSanitizer and UBSan where they link).
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

// an array of a launch: where it lies, its element size and its count
struct Arr {
    const void* p;
    size_t elem, count;
};

// every array inside [base, base + bytes), aligned to its element, and no two overlapping; each
// byte of the block belongs to at most one array.  Returns the bytes covered.
static size_t check_arrays(const std::vector<Arr>& arrs, const char* base, size_t bytes, const char* what) {
    std::vector<unsigned char> owner(bytes, 0);
    size_t covered = 0;
    for (size_t a = 0; a < arrs.size(); ++a) {
        const size_t off = (size_t)((const char*)arrs[a].p - base), len = arrs[a].elem * arrs[a].count;
        CHECK((const char*)arrs[a].p >= base && off + len <= bytes, "%s: array %zu outside the block", what, a);
        CHECK(off % arrs[a].elem == 0, "%s: array %zu at %zu is misaligned", what, a, off);
        if ((const char*)arrs[a].p < base || off + len > bytes) continue;
        for (size_t i = 0; i < len; ++i) {
            CHECK(!owner[off + i], "%s: array %zu overlaps another at byte %zu", what, a, off + i);
            if (owner[off + i]) break;
            owner[off + i] = 1;
        }
        covered += len;
    }
    return covered;
}

static std::vector<Arr> recover_arrays(const RcvParams& c, size_t Q, size_t M, size_t K) {
    const RtmParams& t = c.rt;
    const RjnParams& r = t.rj;
    const HznParams& h = r.hz;
    std::vector<Arr> v;
    for (int i = 0; i < TRAJ_COLS; ++i) v.push_back({h.out[i], 8, Q * M});
    if (M) v.push_back({c.offset, 8, Q * M});
    for (int i = 0; i < HZN_LOC; ++i) v.push_back({h.loc[i], 8, Q});
    for (double* p : {r.scal[0], r.scal[1], t.v_excess, c.scal[0], c.scal[1]}) v.push_back({p, 8, Q});
    for (int32_t* p : {h.seg, h.count, r.merge_node, r.overspeed, t.feasible, t.bind_node, c.clamped, c.offtrack, c.merge_node})
        v.push_back({p, 4, Q});
    for (double* p : {r.node_v, r.node_t, t.node_b, t.node_c, c.node_o, c.node_k}) v.push_back({p, 8, Q * (K + 1)});
    return v;
}

static void check_shape(size_t Q, size_t M, size_t K, size_t C) {
    const QueryLayout L = fan_layout(Q, M, K, C);
    const QueryLayout R = recover_layout(Q, M, K);
    const size_t QC = Q * C;
    // ---- byte counts: the closed forms
    const size_t head_want = (8 * Q * M + 10 * Q + 3 * QC) * 8 + (10 * Q + 2 * Q + 6 * QC) * 4;
    const size_t scratch_want = (10 * QC) * 8 + 10 * QC * 4 + 10 * QC * (K + 1) * 8;
    CHECK(L.C == C && R.C == 0 && L.recover && L.retime && !L.stop, "flags");
    CHECK(L.in_bytes == Q * 48 + QC * 8, "(%zu,%zu,%zu,%zu): in_bytes %zu", Q, M, K, C, L.in_bytes);
    CHECK(L.head_bytes == head_want, "(%zu,%zu,%zu,%zu): head_bytes %zu != %zu", Q, M, K, C, L.head_bytes, head_want);
    CHECK(L.out_bytes == head_want + 6 * Q * (K + 1) * 8, "(%zu,%zu,%zu,%zu): out_bytes %zu", Q, M, K, C, L.out_bytes);
    CHECK(L.scratch_bytes == scratch_want && R.scratch_bytes == 0, "(%zu,%zu,%zu,%zu): scratch_bytes %zu != %zu", Q, M, K, C,
          L.scratch_bytes, scratch_want);
    // ---- without C nothing moves: the recover layout is what it was, and the fan layout's shared part is its
    CHECK(R.in_bytes == Q * 56 && R.head_bytes == (8 * Q * M + 10 * Q) * 8 + 10 * Q * 4 && R.out_bytes == R.head_bytes + 6 * Q * (K + 1) * 8,
          "recover layout: closed forms");
    CHECK(query_layout(Q, M, K, false, true).out_bytes == (7 * Q * M + 8 * Q) * 8 + 6 * Q * 4 + 4 * Q * (K + 1) * 8, "retime layout: closed form");
    CHECK(L.pose == R.pose && L.v0 == R.v0 && L.row == R.row && L.hint == R.hint && L.merge_len == R.merge_len, "the queries' block up to merge_len");
    CHECK(L.dir == L.merge_len + QC * 8, "dir lies behind merge_len [Q][C]");
    for (int c = 0; c < TRAJ_COLS; ++c) CHECK(L.col[c] == R.col[c], "column %d moved", c);
    CHECK(L.offset == R.offset && L.per[0] == R.per[0] && L.cper[1] == R.cper[1], "the columns and the doubles up to hi0");
    CHECK(L.tper[0] == R.cper[1] + Q * 8, "the table's doubles lie behind hi0");
    CHECK(L.nodes[0] == L.head_bytes && L.cnodes[1] + Q * (K + 1) * 8 == L.out_bytes && L.best % 4 == 0 && L.head_bytes % 8 == 0, "head and node arrays");

    // ---- the queries' block
    std::vector<double> pose(2 * Q), v0(Q), len(QC), dir(2 * Q);
    std::vector<int32_t> row(Q), hint(Q);
    for (size_t k = 0; k < Q; ++k) {
        pose[2 * k] = 1000.5 + (double)k;
        pose[2 * k + 1] = -2000.25 - (double)k;
        v0[k] = 3.125 * (double)(k + 1);
        dir[2 * k] = 0.25 * (double)(k + 1);
        dir[2 * k + 1] = -0.5 * (double)(k + 1);
        row[k] = (int32_t)(k + 7);
        hint[k] = (int32_t)(3 * k + 1);
    }
    for (size_t k = 0; k < QC; ++k) len[k] = 10.5 + (double)k;
    rl_cfg cfg{};
    cfg.v_cap_mps = 27.5; cfg.a_lat_max = 9.25; cfg.kappa_eps = 1e-6;
    const double* const bnd[4] = {pose.data(), v0.data(), len.data(), dir.data()};   // (four distinct addresses)
    const rl_fan_query fq{rl_rcv_query{rl_rjn_query{pose.data(), row.data(), hint.data(), (int32_t)Q, 3, (int32_t)M, 0, 0.05, v0.data(),
                                                    &cfg, (int32_t)K, 0},
                                       len.data(), dir.data()},
                          (int32_t)C, 0};
    const rl_stp_query q = as_stp(fq.rc.rj);
    const QueryLayout Lq = fan_layout(fq);
    CHECK(Lq.C == C && Lq.in_bytes == L.in_bytes && Lq.out_bytes == L.out_bytes && Lq.scratch_bytes == L.scratch_bytes, "layout of the query");
    Guarded in(L.in_bytes);
    query_pack(q, L, in.data());
    recover_pack(fq.rc, L, in.data());
    CHECK(std::memcmp(in.data() + L.merge_len, len.data(), QC * 8) == 0, "merge_len [Q][C]");
    CHECK(std::memcmp(in.data() + L.dir, dir.data(), Q * 16) == 0, "dir");
    CHECK(std::memcmp(in.data() + L.pose, pose.data(), Q * 16) == 0 && std::memcmp(in.data() + L.v0, v0.data(), Q * 8) == 0, "pose and v0");
    CHECK(in.intact(), "guard of the queries' block");

    // ---- the launch pointers: the results over exactly out_bytes, the candidates over exactly scratch_bytes
    Guarded out(L.out_bytes), scratch(L.scratch_bytes);
    const StpParams s = query_pointers(q, L, in.data(), out.data());
    const RcvParams w = recover_pointers(retime_pointers(s.rj, cfg, L, out.data()), fq.rc, L, in.data(), out.data(), bnd);
    const FanParams f = fan_pointers(w, cfg, L, out.data(), scratch.data());
    CHECK(f.C == (int32_t)C && f.win.rt.rj.hz.Q == (int32_t)Q && f.cand.rt.rj.hz.Q == (int32_t)QC, "sizes");
    CHECK(f.cand.rt.rj.hz.M_cap == (int32_t)M && f.cand.rt.rj.K_cap == (int32_t)K && f.cand.rt.rj.hz.window == 3 && f.cand.rt.rj.hz.dt == 0.05 &&
              f.cand.rt.v_cap == 27.5,
          "the candidates' launch has the query's sizes and cfg");
    CHECK(f.cand.rt.rj.hz.pose == w.rt.rj.hz.pose && f.cand.rt.rj.v0 == w.rt.rj.v0 && f.cand.rt.rj.hz.row == w.rt.rj.hz.row &&
              f.cand.rt.rj.hz.hint == w.rt.rj.hz.hint && f.cand.merge_len == w.merge_len && f.cand.dir == w.dir && f.cand.lo == bnd[0] &&
              f.cand.ny == bnd[3],
          "the candidates read the query's own arrays and the bounds rows");
    for (size_t k = 0; k < QC; ++k) CHECK(f.win.merge_len[k] == len[k], "merge_len[%zu]", k);
    std::vector<Arr> wa = recover_arrays(f.win, Q, M, K);
    wa.push_back({f.best, 4, Q});
    for (int32_t* p : f.tab_i) wa.push_back({p, 4, QC});
    for (double* p : f.tab_d) wa.push_back({p, 8, QC});
    const size_t wc = check_arrays(wa, out.data(), L.out_bytes, "results");
    CHECK(wc + 2 * Q * 4 == L.out_bytes, "(%zu,%zu,%zu,%zu): the results' arrays and two pad words fill out_bytes: %zu", Q, M, K, C, wc);
    CHECK((const char*)f.tab_d[2] + QC * 8 <= out.data() + L.head_bytes && (const char*)f.tab_i[5] + QC * 4 <= out.data() + L.head_bytes &&
              (const char*)f.win.rt.rj.node_v == out.data() + L.head_bytes,
          "best and the table lie in the head, the node arrays behind it");
    std::vector<Arr> ca = recover_arrays(f.cand, QC, 0, K);
    for (double* p : f.xnode) ca.push_back({p, 8, QC * (K + 1)});
    const size_t cc = check_arrays(ca, scratch.data(), L.scratch_bytes, "scratch");
    CHECK(cc + QC * 4 == L.scratch_bytes, "(%zu,%zu,%zu,%zu): the candidates' arrays and one pad word fill scratch_bytes: %zu", Q, M, K, C, cc);
    // write every element of every array: the guards stay
    for (const std::vector<Arr>* v : {&wa, &ca})
        for (const Arr& a : *v) std::memset((void*)a.p, 0x11, a.elem * a.count);
    CHECK(out.intact() && scratch.intact(), "(%zu,%zu,%zu,%zu): a launch pointer reaches outside its block", Q, M, K, C);

    // ---- the copies out: 0 every field, 1 no node arrays and only the head to read, 2 best and the table alone
    for (size_t k = 0; k < Q; ++k) f.best[k] = (int32_t)(100 + k);
    for (size_t k = 0; k < QC; ++k) {
        for (int c = 0; c < FAN_TAB_INTS; ++c) f.tab_i[c][k] = (int32_t)(1000 * (c + 1) + (int)k);
        for (int c = 0; c < FAN_TAB_SCAL; ++c) f.tab_d[c][k] = 0.5 + 1000.0 * (c + 1) + (double)k;
    }
    for (size_t k = 0; k < Q; ++k) {
        f.win.clamped[k] = (int32_t)(7 + k);
        f.win.scal[1][k] = 9.75 + (double)k;
        f.win.node_k[k * (K + 1) + K] = 2.5 + (double)k;
    }
    for (int variant = 0; variant < 3; ++variant) {
        std::vector<char> src(out.data(), out.data() + (variant == 1 ? L.head_bytes : L.out_bytes));   // exact size
        std::vector<double> col(Q * M, -77.0), per(Q, -77.0), node(Q * (K + 1), -77.0), td[FAN_TAB_SCAL];
        std::vector<int32_t> ints(Q, -77), best(Q, -77), ti[FAN_TAB_INTS];
        for (auto& t : td) t.assign(QC, -77.0);
        for (auto& t : ti) t.assign(QC, -77);
        rl_fan o{};
        if (variant != 2) {
            o.offset = col.data();
            o.clamped = ints.data();
            o.hi0 = per.data();
        }
        if (variant == 0) o.node_k = node.data();
        o.best = best.data();
        o.cand_class = ti[0].data(); o.cand_feasible = ti[1].data(); o.cand_clamped = ti[2].data(); o.cand_merge_node = ti[3].data();
        o.cand_overspeed = ti[4].data(); o.cand_bind_node = ti[5].data();
        o.cand_t_end = td[0].data(); o.cand_t_loss = td[1].data(); o.cand_v_excess = td[2].data();
        CHECK(query_wants_nodes(o) == (variant == 0), "variant %d: query_wants_nodes", variant);
        query_unpack(src.data(), L, o);
        for (size_t k = 0; k < Q; ++k) {
            CHECK(best[k] == (int32_t)(100 + k), "variant %d: best[%zu]", variant, k);
            CHECK(ints[k] == (variant != 2 ? (int32_t)(7 + k) : -77) && per[k] == (variant != 2 ? 9.75 + (double)k : -77.0), "variant %d: clamped / hi0 [%zu]", variant, k);
            CHECK(node[k * (K + 1) + K] == (variant == 0 ? 2.5 + (double)k : -77.0), "variant %d: node_k[%zu]", variant, k);
        }
        for (size_t k = 0; k < QC; ++k) {
            for (int c = 0; c < FAN_TAB_INTS; ++c) CHECK(ti[c][k] == (int32_t)(1000 * (c + 1) + (int)k), "variant %d: table int %d [%zu]", variant, c, k);
            for (int c = 0; c < FAN_TAB_SCAL; ++c) CHECK(td[c][k] == 0.5 + 1000.0 * (c + 1) + (double)k, "variant %d: table double %d [%zu]", variant, c, k);
        }
    }
    CHECK(out.intact(), "guard of the results' block after the copies");
}

int main() {
    const size_t shapes[6][4] = {{1, 1, 1, 1}, {3, 2, 4, 2}, {2, 5, 512, 16}, {65, 7, 9, 5}, {70, 64, 16, 3}, {4096, 1, 1, 16}};
    for (const auto& s : shapes) check_shape(s[0], s[1], s[2], s[3]);
    if (g_bad) {
        std::printf("recover fan layout: %d checks failed\n", g_bad);
        return 1;
    }
    std::printf("recover fan layout ok: 6 shapes\n");
    return 0;
}
