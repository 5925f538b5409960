// Stand-alone check of csrc/rl_query.h, the packed blocks of the six pose-query stages.  One
// harness; argv[1] names the stage (horizon, rejoin, stop, retime, recover, recover_fan), or is
// "dump": every offset and byte count as JSON, in the form of tests/golden/query_layout/offsets.json.
// Per stage and shape: the byte counts of every kind against their closed forms; the offsets beside
// the smaller stage's, which do not move; every byte of the queries' block, with the optional
// arrays given and NULL, and equal to the smaller stage's as far as that goes; the launch pointers
// (by the parameter structs' field names) aligned, on their side of the head, disjoint, filling
// the block and written through between two guard lines; the fan stage's scratch block the same,
// and its candidates' launch on the query's own arrays; and the copies into the stage's results
// struct (by its field names) with every field, with alternating fields NULL, from the head alone,
// with the last node array alone and (fan) with the table alone.  No HIP call; built and run by
// tests/layout_check.py for the five layout tests (under AddressSanitizer and UBSan where they link).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
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
constexpr QueryKind HZN = QueryKind::Horizon, RJN = QueryKind::Rejoin, STP = QueryKind::Stop, RTM = QueryKind::Retime,
                    RCV = QueryKind::Recover, FAN = QueryKind::Fan;

static double dval(int a, size_t q, size_t i) { return (double)(a * 100000000LL + (long long)q * 10000 + (long long)i); }
static int32_t ival(int a, size_t q, size_t i) { return (int32_t)(a * 10000000 + (int)q * 16 + (int)i); }

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

// the shapes of the five programs this one replaces, and the fan stage's C beside each
constexpr size_t SHAPES[7][4] = {{1, 1, 1, 1}, {3, 2, 4, 2}, {2, 5, 1024, 16}, {65, 7, 9, 5}, {2, 5, 512, 16}, {70, 64, 16, 3}, {4096, 1, 1, 16}};

// ---------------------------------------------------------------- what the test states on its own
struct Sizes {
    size_t in, head, out, scratch;
};
// the closed forms of every kind's byte counts
static Sizes closed_forms(QueryKind k, size_t Q, size_t M, size_t K, size_t C) {
    const size_t QC = Q * C, node = Q * (K + 1) * 8;
    switch (k) {
    case HZN: return {Q * 24, (7 * Q * M + 5 * Q) * 8 + 2 * Q * 4, (7 * Q * M + 5 * Q) * 8 + 2 * Q * 4, 0};
    case RJN: return {Q * 32, (7 * Q * M + 7 * Q) * 8 + 4 * Q * 4, (7 * Q * M + 7 * Q) * 8 + 4 * Q * 4 + 2 * node, 0};
    case STP: return {Q * 44, (7 * Q * M + 9 * Q) * 8 + 6 * Q * 4, (7 * Q * M + 9 * Q) * 8 + 6 * Q * 4 + 3 * node, 0};
    case RTM: return {Q * 32, (7 * Q * M + 8 * Q) * 8 + 6 * Q * 4, (7 * Q * M + 8 * Q) * 8 + 6 * Q * 4 + 4 * node, 0};
    case RCV: return {Q * 56, (8 * Q * M + 10 * Q) * 8 + 10 * Q * 4, (8 * Q * M + 10 * Q) * 8 + 10 * Q * 4 + 6 * node, 0};
    case FAN: {
        const size_t head = (8 * Q * M + 10 * Q + 3 * QC) * 8 + (10 * Q + 2 * Q + 6 * QC) * 4;
        return {Q * 48 + QC * 8, head, head + 6 * node, (10 * QC) * 8 + 10 * QC * 4 + 10 * QC * (K + 1) * 8};
    }
    }
    return {};
}
// the smaller stage a kind is laid out beside: none of its offsets moves
static QueryKind neighbour(QueryKind k) { return k == FAN ? RCV : k == RCV ? RTM : k == HZN ? HZN : k == RJN ? HZN : RJN; }
// elements per query of a slot, and whether it holds ints
static size_t width(int s, size_t M, size_t K, size_t C) {
    if (s == S_POSE || s == S_DIR) return 2;
    if (s == S_MERGE_LEN) return C ? C : 1;
    if (s >= S_S && s <= S_OFFSET) return M;
    if ((s >= S_CAND_T_END && s <= S_CAND_V_EXCESS) || (s >= S_CAND_CLASS && s <= S_CAND_BIND_NODE)) return C;
    return s >= S_NODE_V ? K + 1 : 1;
}
static bool is_int(int s) { return s == S_ROW || s == S_HINT || s == S_STOP_SAMPLE || (s >= S_SEG && s <= S_PAD_FAN); }
static bool is_pad(int s) { return s == S_PAD_RCV || s == S_PAD_FAN; }

// ---------------------------------------------------------------- the launch pointers, by name
struct Ptrs {
    void* p[N_SLOTS] = {};
    void hzn(const HznParams& h) {
        for (int c = 0; c < TRAJ_COLS; ++c) p[S_S + c] = h.out[c];
        for (int c = 0; c < HZN_LOC; ++c) p[S_U + c] = h.loc[c];
        p[S_SEG] = h.seg; p[S_COUNT] = h.count;
    }
    void rjn(const RjnParams& r) {
        hzn(r.hz);
        p[S_T_MERGE] = r.scal[0]; p[S_T_LOSS] = r.scal[1];
        p[S_MERGE_NODE] = r.merge_node; p[S_OVERSPEED] = r.overspeed;
        p[S_NODE_V] = r.node_v; p[S_NODE_T] = r.node_t;
    }
    void stp(const StpParams& s) {
        rjn(s.rj);
        p[S_S_STOP] = s.scal[0]; p[S_V_EXCESS] = s.scal[1];
        p[S_REACHABLE] = s.reachable; p[S_BRAKE_NODE] = s.brake_node; p[S_NODE_B] = s.node_b;
    }
    void rtm(const RtmParams& t) {
        rjn(t.rj);
        p[S_V_EXCESS] = t.v_excess; p[S_FEASIBLE] = t.feasible; p[S_BIND_NODE] = t.bind_node;
        p[S_NODE_B] = t.node_b; p[S_NODE_C] = t.node_c;
    }
    void rcv(const RcvParams& c) {
        rtm(c.rt);
        p[S_OFFSET] = c.offset; p[S_LO0] = c.scal[0]; p[S_HI0] = c.scal[1];
        p[S_CLAMPED] = c.clamped; p[S_OFFTRACK] = c.offtrack; p[S_RCV_MERGE_NODE] = c.merge_node;
        p[S_NODE_O] = c.node_o; p[S_NODE_K] = c.node_k;
    }
    void fan(const FanParams& f) {
        rcv(f.win);
        p[S_BEST] = f.best;
        for (int c = 0; c < FAN_TAB_INTS; ++c) p[S_CAND_CLASS + c] = f.tab_i[c];
        for (int c = 0; c < FAN_TAB_SCAL; ++c) p[S_CAND_T_END + c] = f.tab_d[c];
    }
};

// ---------------------------------------------------------------- the results structs, by name
struct Ask {                                     // the destination of every slot, nullptr where not asked
    void* p[N_SLOTS] = {};
};
#define F(f, slot) o.f = (decltype(o.f))a.p[slot]
template <class O>
static void bind_hzn(O& o, const Ask& a) {
    F(s, S_S); F(x, S_X); F(y, S_Y); F(heading, S_HEADING); F(kappa, S_KAPPA); F(v, S_V); F(ax, S_AX);
    F(u, S_U); F(t0, S_T0); F(s0, S_S0); F(e, S_E); F(dist2, S_DIST2); F(seg, S_SEG); F(count, S_COUNT);
}
template <class O>
static void bind_rtm(O& o, const Ask& a) {
    bind_hzn(o, a);
    F(end_node, S_MERGE_NODE); F(overspeed, S_OVERSPEED); F(t_end, S_T_MERGE); F(t_loss, S_T_LOSS); F(node_v, S_NODE_V); F(node_t, S_NODE_T);
    F(feasible, S_FEASIBLE); F(bind_node, S_BIND_NODE); F(v_excess, S_V_EXCESS); F(node_b, S_NODE_B); F(node_c, S_NODE_C);
}
template <class O>
static void bind_rcv(O& o, const Ask& a) {
    bind_rtm(o, a);
    F(offset, S_OFFSET); F(clamped, S_CLAMPED); F(offtrack, S_OFFTRACK); F(merge_node, S_RCV_MERGE_NODE); F(lo0, S_LO0); F(hi0, S_HI0);
    F(node_o, S_NODE_O); F(node_k, S_NODE_K);
}
static void bind(rl_hzn& o, const Ask& a) { bind_hzn(o, a); }
static void bind(rl_rjn& o, const Ask& a) {
    bind_hzn(o, a);
    F(merge_node, S_MERGE_NODE); F(overspeed, S_OVERSPEED); F(t_merge, S_T_MERGE); F(t_loss, S_T_LOSS); F(node_v, S_NODE_V); F(node_t, S_NODE_T);
}
static void bind(rl_stp& o, const Ask& a) {
    bind_hzn(o, a);
    F(stop_node, S_MERGE_NODE); F(overspeed, S_OVERSPEED); F(t_stop, S_T_MERGE); F(v_end, S_T_LOSS); F(node_v, S_NODE_V); F(node_t, S_NODE_T);
    F(reachable, S_REACHABLE); F(brake_node, S_BRAKE_NODE); F(s_stop, S_S_STOP); F(v_excess, S_V_EXCESS); F(node_b, S_NODE_B);
}
static void bind(rl_rtm& o, const Ask& a) { bind_rtm(o, a); }
static void bind(rl_rcv& o, const Ask& a) { bind_rcv(o, a); }
static void bind(rl_fan& o, const Ask& a) {
    bind_rcv(o, a);
    F(best, S_BEST); F(cand_class, S_CAND_CLASS); F(cand_feasible, S_CAND_FEASIBLE); F(cand_clamped, S_CAND_CLAMPED);
    F(cand_merge_node, S_CAND_MERGE_NODE); F(cand_overspeed, S_CAND_OVERSPEED); F(cand_bind_node, S_CAND_BIND_NODE);
    F(cand_t_end, S_CAND_T_END); F(cand_t_loss, S_CAND_T_LOSS); F(cand_v_excess, S_CAND_V_EXCESS);
}
#undef F
template <class O>
static void unpack_as(const char* src, const QueryLayout& L, const Ask& a, bool wants, int variant) {
    O o{};
    bind(o, a);
    CHECK(query_wants_nodes(L.kind, &o) == wants, "%s variant %d: query_wants_nodes", kind_info(L.kind).name, variant);
    query_unpack(src, L, &o);
}

// ---------------------------------------------------------------- arrays of a block
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

// ---------------------------------------------------------------- one stage, one shape
static void check_shape(QueryKind kind, size_t Q, size_t M, size_t Kq, size_t Cq) {
    const size_t K = kind == HZN ? 0 : Kq, C = kind == FAN ? Cq : 0, QC = Q * C;
    const char* name = kind_info(kind).name;
    const QueryLayout L = query_layout_of(kind, Q, M, K, C);
    const QueryKind nk = neighbour(kind);
    const QueryLayout N = query_layout_of(nk, Q, M, nk == HZN ? 0 : K);
#define AT "%s (%zu,%zu,%zu,%zu): "
#define ATV name, Q, M, K, C

    // ---- byte counts: the closed forms, of this kind and of every other beside it
    for (int k = 0; k < QUERY_KINDS; ++k) {
        const QueryKind o = (QueryKind)k;
        const size_t Ko = o == HZN ? 0 : Kq, Co = o == FAN ? Cq : 0;
        const QueryLayout X = query_layout_of(o, Q, M, Ko, Co);
        const Sizes w = closed_forms(o, Q, M, Ko, Co);
        CHECK(X.in_bytes == w.in && X.head_bytes == w.head && X.out_bytes == w.out && X.scratch_bytes == w.scratch,
              AT "%s: bytes %zu %zu %zu %zu, closed forms %zu %zu %zu %zu", ATV, kind_info(o).name, X.in_bytes, X.head_bytes, X.out_bytes,
              X.scratch_bytes, w.in, w.head, w.out, w.scratch);
        CHECK(X.kind == o && X.Q == Q && X.M == M && X.K == Ko && X.C == Co, AT "%s: sizes and kind", ATV, kind_info(o).name);
    }
    // ---- beside the smaller stage nothing moves: in either block, every array both have lies where
    // it lay, up to the first array that only this kind has
    size_t in_same = 0;                              // the bytes of the queries' block both lay out alike
    for (int s = 0, moved = 0; s < N_SLOTS && kind != HZN; ++s) {
        if (s == S_OUT_FIRST) moved = 0;
        if (L.bytes[s] != N.bytes[s]) moved = 1;
        if (!moved) CHECK(L.off[s] == N.off[s], AT "%s moved beside the %s stage's", ATV, kSlots[s].name, kind_info(nk).name);
        if (!moved && s < S_OUT_FIRST) in_same = L.off[s] + L.bytes[s];
    }
    const size_t node = Q * (K + 1) * 8;
    CHECK(L.has(S_S) && L.has(S_SEG) && L.has(S_V0) == (kind != HZN) && L.has(S_STOP_SAMPLE) == (kind == STP) &&
              L.has(S_NODE_C) == (kind == RTM || kind == RCV || kind == FAN) && L.has(S_NODE_K) == (kind == RCV || kind == FAN) &&
              L.has(S_BEST) == (kind == FAN),
          AT "the arrays the kind has", ATV);
    if (kind != HZN) CHECK(L.off[S_NODE_V] == L.head_bytes && L.off[S_NODE_V] % 8 == 0, AT "node_v begins the node side", ATV);
    if (kind == STP) {
        CHECK(N.in_bytes == Q * 32 && L.off[S_V_TARGET] == N.in_bytes && L.off[S_V_TARGET] % 8 == 0 && L.off[S_STOP_SAMPLE] % 4 == 0, AT "queries' block", ATV);
        CHECK(L.off[S_NODE_B] % 8 == 0 && L.off[S_S_STOP] % 8 == 0 && L.off[S_V_EXCESS] % 8 == 0, AT "alignment", ATV);
    }
    if (kind == RTM) {
        CHECK(L.in_bytes == N.in_bytes, AT "the queries' block is the rejoin stage's", ATV);
        for (int s = S_S; s <= S_T_LOSS; ++s) CHECK(!L.has((Slot)s) || L.off[s] == N.off[s], AT "%s moved", ATV, kSlots[s].name);
        CHECK(L.off[S_V_EXCESS] == N.off[S_T_LOSS] + Q * 8 && L.off[S_V_EXCESS] % 8 == 0, AT "v_excess lies behind the rejoin stage's doubles", ATV);
        CHECK(L.off[S_FEASIBLE] % 4 == 0 && L.off[S_BIND_NODE] == L.off[S_FEASIBLE] + Q * 4 && L.off[S_BIND_NODE] + Q * 4 == L.head_bytes,
              AT "the ints end the head", ATV);
        CHECK(L.off[S_NODE_B] == L.off[S_NODE_T] + node && L.off[S_NODE_C] + node == L.out_bytes && L.off[S_NODE_B] % 8 == 0 && L.off[S_NODE_C] % 8 == 0,
              AT "node arrays", ATV);
    }
    if (kind == RCV) {
        CHECK(L.off[S_MERGE_LEN] == N.in_bytes && L.off[S_DIR] == L.off[S_MERGE_LEN] + Q * 8 && L.off[S_MERGE_LEN] % 8 == 0,
              AT "merge_len and dir lie behind hint", ATV);
        CHECK(L.off[S_OFFSET] == 7 * Q * M * 8, AT "offset lies behind the seven columns", ATV);
        CHECK(L.off[S_NODE_K] + node == L.out_bytes, AT "node arrays", ATV);
    }
    if (kind == FAN) {
        CHECK(L.off[S_MERGE_LEN] == N.off[S_MERGE_LEN] && L.off[S_DIR] == L.off[S_MERGE_LEN] + QC * 8, AT "dir lies behind merge_len [Q][C]", ATV);
        CHECK(L.off[S_OFFSET] == N.off[S_OFFSET] && L.off[S_U] == N.off[S_U] && L.off[S_HI0] == N.off[S_HI0], AT "the columns and the doubles up to hi0", ATV);
        CHECK(L.off[S_CAND_T_END] == N.off[S_HI0] + Q * 8, AT "the table's doubles lie behind hi0", ATV);
        CHECK(L.off[S_NODE_K] + node == L.out_bytes && L.off[S_BEST] % 4 == 0 && L.head_bytes % 8 == 0, AT "head and node arrays", ATV);
        CHECK(N.scratch_bytes == 0, AT "a recover stage has no scratch block", ATV);
    }

    // ---- the queries' block: every byte, built from the documented order alone, with the optional
    // arrays given and NULL; and equal to the smaller stage's as far as both are laid out alike
    std::vector<double> pose(2 * Q), v0(Q), vt(Q), len(Q * (C ? C : 1)), dir(2 * Q);
    std::vector<int32_t> row(Q), hint(Q), js(Q);
    for (size_t k = 0; k < Q; ++k) {
        pose[2 * k] = 1000.5 + (double)k;
        pose[2 * k + 1] = -2000.25 - (double)k;
        v0[k] = 3.125 * (double)(k + 1);
        vt[k] = 0.5 * (double)(k + 3);
        dir[2 * k] = 0.25 * (double)(k + 1);
        dir[2 * k + 1] = -0.5 * (double)(k + 1);
        row[k] = (int32_t)(k + 7);
        hint[k] = (int32_t)(3 * k + 1);
        js[k] = (int32_t)(5 * k + 2);
    }
    for (size_t k = 0; k < len.size(); ++k) len[k] = 10.5 + (double)k;
    rl_cfg cfg{};
    cfg.v_cap_mps = 27.5; cfg.a_lat_max = 9.25; cfg.kappa_eps = 1e-6;
    Guarded in(L.in_bytes), in_n(N.in_bytes);
    QueryView q{};
    for (int given = 1; given >= 0; --given) {   // (the last pass leaves the optional arrays NULL; packed again below)
        const int32_t* rw = given ? row.data() : nullptr;
        const int32_t* hn = given ? hint.data() : nullptr;
        const rl_rjn_query rj{pose.data(), rw, hn, (int32_t)Q, 3, (int32_t)M, 0, 0.05, v0.data(), &cfg, (int32_t)K, 0};
        switch (kind) {
        case HZN: q = query_view(rl_hzn_query{pose.data(), rw, hn, (int32_t)Q, 3, (int32_t)M, 0, 0.05}); break;
        case RJN: q = query_view(rj); break;
        case STP: q = query_view(rl_stp_query{rj, js.data(), given ? vt.data() : nullptr}); break;
        case RTM: q = query_view(rl_rtm_query{rj}); break;
        case RCV: q = query_view(rl_rcv_query{rj, len.data(), given ? dir.data() : nullptr}); break;
        case FAN: q = query_view(rl_fan_query{rl_rcv_query{rj, len.data(), given ? dir.data() : nullptr}, (int32_t)C, 0}); break;
        }
        const QueryLayout Lq = query_layout_of(kind, q);
        CHECK(Lq.kind == kind && Lq.C == C && Lq.in_bytes == L.in_bytes && Lq.head_bytes == L.head_bytes && Lq.out_bytes == L.out_bytes &&
                  Lq.scratch_bytes == L.scratch_bytes && std::memcmp(Lq.off, L.off, sizeof L.off) == 0,
              AT "layout of the query", ATV);
        std::memset(in.data(), FILL, L.in_bytes);
        query_pack(q, L, in.data());
        std::vector<unsigned char> want(closed_forms(kind, Q, M, K, C).in, FILL);
        unsigned char* w = want.data();
        std::memcpy(w, pose.data(), Q * 16); w += Q * 16;
        if (kind != HZN) { std::memcpy(w, v0.data(), Q * 8); w += Q * 8; }
        for (size_t k = 0; k < Q; ++k, w += 4) { const int32_t r = given ? row[k] : 0; std::memcpy(w, &r, 4); }
        for (size_t k = 0; k < Q; ++k, w += 4) { const int32_t g = given ? hint[k] : -1; std::memcpy(w, &g, 4); }
        if (kind == STP) {
            for (size_t k = 0; k < Q; ++k, w += 8) { const double t = given ? vt[k] : 0.0; std::memcpy(w, &t, 8); }
            std::memcpy(w, js.data(), Q * 4); w += Q * 4;
        }
        if (kind == RCV || kind == FAN) {
            std::memcpy(w, len.data(), len.size() * 8); w += len.size() * 8;
            if (given) std::memcpy(w, dir.data(), Q * 16);     // (a NULL dir_xy leaves that part unwritten)
            w += Q * 16;
        }
        CHECK(w == want.data() + want.size() && want.size() == L.in_bytes, AT "expected block size", ATV);
        CHECK(std::memcmp(in.data(), want.data(), want.size()) == 0, AT "given=%d: queries' block differs", ATV, given);
        std::memset(in_n.data(), FILL, N.in_bytes);
        query_pack(q, N, in_n.data());
        CHECK(in_same <= N.in_bytes && std::memcmp(in.data(), in_n.data(), in_same) == 0, AT "the queries' block differs from the %s stage's", ATV,
              kind_info(nk).name);
        if (kind == RTM || kind == RCV) CHECK(in_same == N.in_bytes, AT "the smaller stage's whole block", ATV);
        CHECK(in.intact() && in_n.intact(), AT "guard of the queries' block", ATV);
        if (kind == RCV || kind == FAN) {
            const double* const b4[4] = {pose.data(), v0.data(), len.data(), dir.data()};
            Guarded o2(L.out_bytes);
            const RcvParams c = recover_pointers(retime_pointers(query_pointers(q.rj, L, in.data(), o2.data()), cfg, L, o2.data()), q.dir_xy != nullptr,
                                                 L, in.data(), o2.data(), b4);
            CHECK((c.dir != nullptr) == (given != 0), AT "a NULL dir_xy gives a null dir", ATV);
        }
    }
    q.rj.row = row.data(); q.rj.seg_hint = hint.data();
    if (kind == STP) q.v_target = vt.data();
    if (kind == RCV || kind == FAN) q.dir_xy = dir.data();
    query_pack(q, L, in.data());

    // ---- the launch pointers over exactly out_bytes (and scratch_bytes)
    Guarded out(L.out_bytes), scratch(L.scratch_bytes);
    const double* const bnd[4] = {pose.data(), v0.data(), len.data(), dir.data()};   // (four distinct addresses)
    const RjnParams r = query_pointers(q.rj, L, in.data(), out.data());
    const HznParams& h = r.hz;
    Ptrs P;
    FanParams f{};
    CHECK(h.Q == (int32_t)Q && h.M_cap == (int32_t)M && h.window == 3 && h.dt == 0.05 && r.K_cap == (int32_t)K, AT "sizes", ATV);
    for (size_t k = 0; k < Q; ++k) {
        CHECK(h.pose[2 * k] == pose[2 * k] && h.pose[2 * k + 1] == pose[2 * k + 1], AT "pose[%zu]", ATV, k);
        CHECK(h.row[k] == row[k] && h.hint[k] == hint[k], AT "row / hint[%zu]", ATV, k);
        if (kind != HZN) CHECK(r.v0[k] == v0[k], AT "v0[%zu]", ATV, k);
    }
    if (kind == HZN) {
        CHECK(!r.v0 && !r.scal[0] && !r.scal[1] && !r.merge_node && !r.overspeed && !r.node_v && !r.node_t, "horizon: rejoin pointers");
        P.hzn(h);
    } else if (kind == RJN) {
        P.rjn(r);
    } else if (kind == STP) {
        const StpParams s = stop_pointers(r, L, in.data(), out.data());
        for (size_t k = 0; k < Q; ++k) CHECK(s.v_target[k] == vt[k] && s.stop_sample[k] == js[k], AT "v_target / stop_sample[%zu]", ATV, k);
        P.stp(s);
    } else {
        const RtmParams t = retime_pointers(r, cfg, L, out.data());
        CHECK(t.v_cap == 27.5 && t.a_lat_max == 9.25 && t.kappa_eps == 1e-6, AT "the ceiling's cfg fields", ATV);
        if (kind == RTM) P.rtm(t);
        else {
            const RcvParams c = recover_pointers(t, true, L, in.data(), out.data(), bnd);
            CHECK(c.lo == bnd[0] && c.hi == bnd[1] && c.nx == bnd[2] && c.ny == bnd[3], AT "the bounds rows", ATV);
            for (size_t k = 0; k < len.size(); ++k) CHECK(c.merge_len[k] == len[k], AT "merge_len[%zu]", ATV, k);
            for (size_t k = 0; k < Q; ++k) CHECK(c.dir[2 * k] == dir[2 * k] && c.dir[2 * k + 1] == dir[2 * k + 1], AT "dir[%zu]", ATV, k);
            if (kind == RCV) P.rcv(c);
            else {
                f = fan_pointers(c, cfg, L, out.data(), scratch.data());
                P.fan(f);
            }
        }
    }
    std::vector<Arr> wa;
    size_t pads = 0;
    for (int s = S_OUT_FIRST; s < N_SLOTS; ++s) {
        if (is_pad(s)) { pads += L.bytes[s]; continue; }
        CHECK((P.p[s] != nullptr) == L.has((Slot)s), AT "%s: a launch pointer exactly where the kind has the array", ATV, kSlots[s].name);
        if (!P.p[s] || !L.has((Slot)s)) continue;
        const size_t off = (size_t)((const char*)P.p[s] - out.data()), wd = width(s, M, K, C);
        CHECK(off == L.off[s], AT "%s: the pointer is not at the slot's offset", ATV, kSlots[s].name);
        CHECK(off % (is_int(s) ? 4 : 8) == 0, AT "%s at %zu is misaligned", ATV, kSlots[s].name, off);
        CHECK(s < S_NODE_FIRST ? off + Q * wd * (is_int(s) ? 4 : 8) <= L.head_bytes : off >= L.head_bytes, AT "%s on the wrong side of the head", ATV,
              kSlots[s].name);
        wa.push_back({P.p[s], (size_t)(is_int(s) ? 4 : 8), Q * wd});
    }
    const size_t wc = check_arrays(wa, out.data(), L.out_bytes, "results");
    CHECK(pads == Q * 4 * ((kind == RCV || kind == FAN) + (kind == FAN)) && wc + pads == L.out_bytes,
          AT "the results' arrays and the pad words fill out_bytes: %zu + %zu", ATV, wc, pads);
    for (int s = S_OUT_FIRST; s < N_SLOTS; ++s)
        for (size_t k = 0; P.p[s] && k < Q; ++k)
            for (size_t i = 0, wd = width(s, M, K, C); i < wd; ++i) {
                if (is_int(s)) ((int32_t*)P.p[s])[k * wd + i] = ival(s, k, i);
                else ((double*)P.p[s])[k * wd + i] = dval(s, k, i);
            }
    CHECK(out.intact(), AT "a launch pointer reaches outside out_bytes", ATV);

    // ---- the fan stage's scratch block and its candidates' launch
    if (kind == FAN) {
        const RcvParams& w = f.win;
        CHECK(f.C == (int32_t)C && f.win.rt.rj.hz.Q == (int32_t)Q && f.cand.rt.rj.hz.Q == (int32_t)QC, AT "sizes", ATV);
        CHECK(f.cand.rt.rj.hz.M_cap == (int32_t)M && f.cand.rt.rj.K_cap == (int32_t)K && f.cand.rt.rj.hz.window == 3 && f.cand.rt.rj.hz.dt == 0.05 &&
                  f.cand.rt.v_cap == 27.5,
              AT "the candidates' launch has the query's sizes and cfg", ATV);
        CHECK(f.cand.rt.rj.hz.pose == w.rt.rj.hz.pose && f.cand.rt.rj.v0 == w.rt.rj.v0 && f.cand.rt.rj.hz.row == w.rt.rj.hz.row &&
                  f.cand.rt.rj.hz.hint == w.rt.rj.hz.hint && f.cand.merge_len == w.merge_len && f.cand.dir == w.dir && f.cand.lo == bnd[0] &&
                  f.cand.hi == bnd[1] && f.cand.nx == bnd[2] && f.cand.ny == bnd[3],
              AT "the candidates read the query's own arrays and the bounds rows", ATV);
        CHECK(f.cand.offset == nullptr, AT "the candidates have no ticks", ATV);
        Ptrs S;
        S.rcv(f.cand);
        std::vector<Arr> ca;
        for (int s = S_OUT_FIRST; s < N_SLOTS; ++s) {
            const bool want = (kSlots[s].kinds & kbit(RCV)) != 0 && !is_pad(s) && s != S_OFFSET;
            CHECK((S.p[s] != nullptr) == want, AT "%s: a candidates' pointer exactly where a recover stage has the array", ATV, kSlots[s].name);
            if (S.p[s]) ca.push_back({S.p[s], (size_t)(is_int(s) ? 4 : 8), QC * width(s, 0, K, 0)});
        }
        for (double* p : f.xnode) ca.push_back({p, 8, QC * (K + 1)});
        const size_t cc = check_arrays(ca, scratch.data(), L.scratch_bytes, "scratch");
        CHECK(cc + QC * 4 == L.scratch_bytes, AT "the candidates' arrays and one pad word fill scratch_bytes: %zu", ATV, cc);
        for (const Arr& a : ca) std::memset((void*)a.p, 0x11, a.elem * a.count);   // write every element: the guards stay
        CHECK(out.intact() && scratch.intact(), AT "a candidates' pointer reaches outside the scratch block", ATV);
    }

    // ---- the copies out: 0 every field, 1 / 2 alternating fields NULL, 3 no node arrays and only the
    // head to read, 4 the last node array alone, 5 (fan) best and the table alone
    int last_node = -1;
    for (int s = S_NODE_FIRST; s < N_SLOTS; ++s)
        if (L.has((Slot)s)) last_node = s;
    for (int variant = 0; variant < 6; ++variant) {
        if ((variant == 4 && last_node < 0) || (variant == 5 && kind != FAN)) continue;
        const bool head_only = variant == 3 || variant == 5;
        std::vector<char> src(out.data(), out.data() + (head_only ? L.head_bytes : L.out_bytes));   // exact size
        std::vector<double> dd[N_SLOTS];
        std::vector<int32_t> di[N_SLOTS];
        bool asked[N_SLOTS] = {};
        Ask a;
        bool wants = false;
        for (int s = S_OUT_FIRST; s < N_SLOTS; ++s) {
            if (!L.has((Slot)s) || is_pad(s)) continue;
            const size_t n = Q * width(s, M, K, C);
            if (is_int(s)) di[s].assign(n, -77);
            else dd[s].assign(n, -77.0);
            asked[s] = variant == 0 || (variant == 3 ? s < S_NODE_FIRST : variant == 4 ? s == last_node
                                        : variant == 5 ? s == S_BEST || width(s, 0, 0, 2) == 2 : s % 2 == variant - 1);
            if (asked[s]) a.p[s] = is_int(s) ? (void*)di[s].data() : (void*)dd[s].data();
            wants = wants || (asked[s] && s >= S_NODE_FIRST);
        }
        CHECK(wants == (variant != 3 && variant != 5 && last_node >= 0), AT "variant %d asks for node arrays", ATV, variant);
        switch (kind) {
        case HZN: unpack_as<rl_hzn>(src.data(), L, a, wants, variant); break;
        case RJN: unpack_as<rl_rjn>(src.data(), L, a, wants, variant); break;
        case STP: unpack_as<rl_stp>(src.data(), L, a, wants, variant); break;
        case RTM: unpack_as<rl_rtm>(src.data(), L, a, wants, variant); break;
        case RCV: unpack_as<rl_rcv>(src.data(), L, a, wants, variant); break;
        case FAN: unpack_as<rl_fan>(src.data(), L, a, wants, variant); break;
        }
        for (int s = S_OUT_FIRST; s < N_SLOTS; ++s)
            for (size_t k = 0; k < Q && (dd[s].size() || di[s].size()); ++k)
                for (size_t i = 0, wd = width(s, M, K, C); i < wd; ++i) {
                    if (is_int(s)) {
                        const int32_t want = asked[s] ? ival(s, k, i) : -77;
                        CHECK(di[s][k * wd + i] == want, AT "variant %d: %s [%zu][%zu] = %d, not %d", ATV, variant, kSlots[s].name, k, i, di[s][k * wd + i], want);
                    } else {
                        const double want = asked[s] ? dval(s, k, i) : -77.0;
                        CHECK(dd[s][k * wd + i] == want, AT "variant %d: %s [%zu][%zu] = %.17g, not %.17g", ATV, variant, kSlots[s].name, k, i,
                              dd[s][k * wd + i], want);
                    }
                }
    }
    CHECK(out.intact(), AT "guard of the results' block after the copies", ATV);
#undef AT
#undef ATV
}

// every offset and byte count of every kind over SHAPES (the fan stage with C in {1, 3, 16}), in the
// golden file's form; the pad words have no entry
static void dump() {
    std::printf("{\"slots\": [");
    bool first = true;
    for (int s = 0; s < N_SLOTS; ++s)
        if (!is_pad(s)) { std::printf("%s\"%s\"", first ? "" : ", ", kSlots[s].name); first = false; }
    std::printf("],\n \"layouts\": [\n");
    first = true;
    const size_t fanC[3] = {1, 3, 16};
    for (int k = 0; k < QUERY_KINDS; ++k)
        for (const auto& sh : SHAPES)
            for (int ci = 0; ci < ((QueryKind)k == FAN ? 3 : 1); ++ci) {
                const QueryLayout L = query_layout_of((QueryKind)k, sh[0], sh[1], (QueryKind)k == HZN ? 0 : sh[2], (QueryKind)k == FAN ? fanC[ci] : 0);
                std::printf("%s  {\"kind\": \"%s\", \"Q\": %zu, \"M\": %zu, \"K\": %zu, \"C\": %zu, \"in_bytes\": %zu, \"head_bytes\": %zu, "
                            "\"out_bytes\": %zu, \"scratch_bytes\": %zu,\n   \"off\": [",
                            first ? "" : ",\n", kKinds[k].name, L.Q, L.M, L.K, L.C, L.in_bytes, L.head_bytes, L.out_bytes, L.scratch_bytes);
                first = false;
                bool f1 = true;
                for (int s = 0; s < N_SLOTS; ++s) {
                    if (is_pad(s)) continue;
                    std::printf("%s%lld", f1 ? "" : ", ", L.has((Slot)s) ? (long long)L.off[s] : -1LL);
                    f1 = false;
                }
                std::printf("]}");
            }
    std::printf("\n ]}\n");
}

int main(int argc, char** argv) {
    const std::string stage = argc > 1 ? argv[1] : "";
    if (stage == "dump") {
        dump();
        return 0;
    }
    int kind = -1;
    for (int k = 0; k < QUERY_KINDS; ++k)
        if (stage == kKinds[k].name) kind = k;
    if (kind < 0) {
        std::printf("usage: query_layout_check horizon|rejoin|stop|retime|recover|recover_fan|dump\n");
        return 2;
    }
    for (const auto& s : SHAPES) check_shape((QueryKind)kind, s[0], s[1], s[2], s[3]);
    if (g_bad) {
        std::printf("%s layout: %d checks failed\n", kKinds[kind].name, g_bad);
        return 1;
    }
    std::printf("%s layout ok: %zu shapes\n", kKinds[kind].name, sizeof(SHAPES) / sizeof(SHAPES[0]));
    return 0;
}
