// rl_query.h — the packed blocks of the pose-query stages (horizon; rejoin, §3m;
// stop, §3n): where every array lies, and the host code that fills the queries' block, points a
// launch at both blocks and copies a results' block out.  The horizon stage is the rejoin stage
// with the optional parts empty, so both go through the rejoin forms (as_rjn) with K = K_cap =
// 0 for the horizon.  The stop stage is the rejoin stage with a target and more results: its
// forms (as_stp) hold the rejoin forms, and a layout with `stop` set has the extra arrays, each
// kind behind the rejoin stage's of that kind; without it no offset or byte count moves.  The
// retime stage (§3p) is the rejoin stage with more results: its query is the rejoin stage's, and
// a layout with `retime` set has its extra arrays in the same places; without it no offset or
// byte count moves.  No HIP call: a host compiler builds it without a device
// (tests/test_query_layout_cpu.py, tests/test_stop_layout_cpu.py, tests/test_retime_cpu.py).
// The recover stage (§3q) is the retime stage with a merge length and a direction per query and
// more results: recover_layout is the retime layout with its extra arrays, again each kind behind
// the others of that kind (tests/test_recover_cpu.py).  The fan stage (§3r) is the recover stage
// with C merge lengths per query and a table of the candidates: fan_layout is the recover layout
// with merge_len [Q][C] and the table behind the others of its kind, and a scratch block for the
// candidates beside the two (tests/test_recover_fan_cpu.py).  Not part of the public ABI.
#pragma once
#include <cstddef>
#include <cstring>

#include "rl_abi.h"
#include "rl_rejoin.h"
#include "rl_stop.h"
#include "rl_retime.h"
#include "rl_recover.h"
#include "rl_recover_fan.h"

namespace rl {

constexpr int QRY_PER = HZN_LOC + RJN_SCAL;   // u, t0, s0, e, dist2, t_merge, t_loss
constexpr int QRY_INTS = 4;                   // seg, count, merge_node, overspeed
constexpr int QRY_NODES = 2;                  // node_v, node_t

// Byte offsets of the arrays of a stage of Q queries, M ticks and K nodes.  The queries' block:
// pose [Q][2], v0 [Q] (rejoin), row [Q], hint [Q].  The results' block: the columns [Q][M] in
// rl_hzn's order, the n_per doubles [Q], the n_ints ints [Q] (the head, always downloaded), the
// n_nodes node arrays [Q][K + 1].  A stop stage's blocks have as well: v_target [Q] and
// stop_sample [Q] behind hint; s_stop and v_excess [Q] behind the n_per doubles, reachable and
// brake_node [Q] behind the n_ints ints (all four in the head), node_b [Q][K + 1] behind the
// node arrays.  Its stop_node, t_stop and v_end lie where the rejoin stage's merge_node,
// t_merge and t_loss do.  A retime stage's results' block has as well: v_excess [Q] behind the
// n_per doubles, feasible and bind_node [Q] behind the n_ints ints (all three in the head),
// node_b and node_c [Q][K + 1] behind the node arrays.  Its end_node and t_end lie where the
// rejoin stage's merge_node and t_merge do.  A recover stage's blocks (recover_layout; `retime`
// set as well) have as well: merge_len [Q] and dir [Q][2] behind hint; the column offset [Q][M]
// behind the seven; lo0, hi0 [Q] behind the doubles and clamped, offtrack, merge_node [Q] and one
// pad word per query (the node arrays stay 8-byte aligned) behind the ints (all in the head);
// node_o, node_k [Q][K + 1] behind the node arrays.  A fan stage's blocks (fan_layout; C > 0, and
// `retime` and `recover` set) have merge_len [Q][C]; the table's doubles [Q][C] behind the doubles;
// best [Q], the table's ints [Q][C] and one more pad word per query behind the recover stage's pad
// (all in the head).  Its scratch block (scratch_bytes, on the device only) is the results' block
// of a recover stage of Q*C queries without ticks, then P.x, P.y, d', psi [Q*C][K + 1].
struct QueryLayout {
    size_t Q, M, K;
    size_t pose, v0, row, hint, in_bytes;
    int n_per, n_ints, n_nodes;
    size_t col[TRAJ_COLS], per[QRY_PER], ints[QRY_INTS], nodes[QRY_NODES], head_bytes, out_bytes;
    bool stop;
    size_t v_target, stop_sample, sper[STP_SCAL], sints[STP_INTS], node_b;
    bool retime;
    size_t rper[RTM_SCAL], rints[RTM_INTS], rnodes[RTM_NODES];
    bool recover;
    size_t merge_len, dir, offset, cper[RCV_SCAL], cints[RCV_INTS], cnodes[RCV_NODES];
    size_t C;                                  // candidates per query; 0: no fan stage's
    size_t best, tper[FAN_TAB_SCAL], tints[FAN_TAB_INTS], scratch_bytes;
};

// every stage's layout; `recover` adds the recover stage's arrays to a retime layout, C > 0 the
// fan stage's to a recover layout
inline QueryLayout query_layout_of(size_t Q, size_t M, size_t K, bool stop, bool retime, bool recover, size_t C = 0) {
    QueryLayout L{};
    L.C = C;
    const bool rjn = K > 0;
    L.Q = Q; L.M = M; L.K = K;
    L.stop = stop;
    L.retime = retime;
    L.recover = recover;
    L.n_per = HZN_LOC + (rjn ? RJN_SCAL : 0);
    L.n_ints = rjn ? QRY_INTS : 2;
    L.n_nodes = rjn ? QRY_NODES : 0;
    size_t at = 0;                             // the cursor
    auto take = [&at](size_t bytes) { const size_t o = at; at += bytes; return o; };
    L.pose = take(Q * 16);
    L.v0 = take(rjn ? Q * 8 : 0);
    L.row = take(Q * 4);
    L.hint = take(Q * 4);
    L.v_target = take(stop ? Q * 8 : 0);
    L.stop_sample = take(stop ? Q * 4 : 0);
    L.merge_len = take(recover ? Q * (C ? C : 1) * 8 : 0);
    L.dir = take(recover ? Q * 16 : 0);
    L.in_bytes = at;
    at = 0;
    for (auto& o : L.col) o = take(Q * M * 8);
    L.offset = take(recover ? Q * M * 8 : 0);
    for (int c = 0; c < L.n_per; ++c) L.per[c] = take(Q * 8);
    for (auto& o : L.sper) o = take(stop ? Q * 8 : 0);
    for (auto& o : L.rper) o = take(retime ? Q * 8 : 0);
    for (auto& o : L.cper) o = take(recover ? Q * 8 : 0);
    for (auto& o : L.tper) o = take(Q * C * 8);
    for (int c = 0; c < L.n_ints; ++c) L.ints[c] = take(Q * 4);
    for (auto& o : L.sints) o = take(stop ? Q * 4 : 0);
    for (auto& o : L.rints) o = take(retime ? Q * 4 : 0);
    for (auto& o : L.cints) o = take(recover ? Q * 4 : 0);
    static_assert(RCV_INTS % 2 == 1, "the pad below keeps the node arrays 8-byte aligned");
    take(recover ? Q * 4 : 0);
    L.best = take(C ? Q * 4 : 0);
    for (auto& o : L.tints) o = take(Q * C * 4);
    static_assert(FAN_TAB_INTS % 2 == 0, "best and the pad below keep the node arrays 8-byte aligned");
    take(C ? Q * 4 : 0);
    L.head_bytes = at;
    for (int c = 0; c < L.n_nodes; ++c) L.nodes[c] = take(Q * (K + 1) * 8);
    L.node_b = take(stop ? Q * (K + 1) * 8 : 0);
    for (auto& o : L.rnodes) o = take(retime ? Q * (K + 1) * 8 : 0);
    for (auto& o : L.cnodes) o = take(recover ? Q * (K + 1) * 8 : 0);
    L.out_bytes = at;
    if (C) L.scratch_bytes = query_layout_of(Q * C, 0, K, false, true, true).out_bytes + FAN_XNODES * (Q * C) * (K + 1) * 8;
    return L;
}
inline QueryLayout query_layout(size_t Q, size_t M, size_t K, bool stop = false, bool retime = false) {
    return query_layout_of(Q, M, K, stop, retime, false);
}
// a recover stage's: the retime layout of a rejoin query with the recover stage's arrays
inline QueryLayout recover_layout(size_t Q, size_t M, size_t K) { return query_layout_of(Q, M, K, false, true, true); }

// a horizon query and its results in the rejoin forms: no v0, no cfg, K_cap = 0, the extra
// fields NULL
inline rl_rjn_query as_rjn(const rl_hzn_query& q) {
    return {q.pose_xy, q.row, q.seg_hint, q.Q, q.window, q.M_cap, 0, q.dt, nullptr, nullptr, 0, 0};
}
inline rl_rjn as_rjn(const rl_hzn& o) {
    return {o.s, o.x, o.y, o.heading, o.kappa, o.v, o.ax, o.u, o.t0, o.s0, o.e, o.dist2, o.seg, o.count,
            nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
}
inline QueryLayout query_layout(const rl_rjn_query& q) { return query_layout((size_t)q.Q, (size_t)q.M_cap, (size_t)q.K_cap); }

// a horizon or rejoin query and its results in the stop forms: no target, the extra fields
// NULL; and the rejoin part of a stop stage's results (rl_stp begins with rl_rjn's fields)
inline rl_stp_query as_stp(const rl_rjn_query& q) { return {q, nullptr, nullptr}; }
inline rl_rjn as_rjn(const rl_stp& o) {
    return {o.s, o.x, o.y, o.heading, o.kappa, o.v, o.ax, o.u, o.t0, o.s0, o.e, o.dist2, o.seg, o.count,
            o.stop_node, o.overspeed, o.t_stop, o.v_end, o.node_v, o.node_t};
}
inline rl_stp as_stp(const rl_rjn& o) {
    return {o.s, o.x, o.y, o.heading, o.kappa, o.v, o.ax, o.u, o.t0, o.s0, o.e, o.dist2, o.seg, o.count,
            o.merge_node, o.overspeed, o.t_merge, o.t_loss, o.node_v, o.node_t,
            nullptr, nullptr, nullptr, nullptr, nullptr};
}
// a query with a stop_sample is a stop stage's; retime: the rejoin query of a retime stage
inline QueryLayout query_layout(const rl_stp_query& q, bool retime = false) {
    return query_layout((size_t)q.rj.Q, (size_t)q.rj.M_cap, (size_t)q.rj.K_cap, q.stop_sample != nullptr, retime);
}
// the rejoin part of a retime stage's results (rl_rtm begins with rl_rjn's fields)
inline rl_rjn as_rjn(const rl_rtm& o) {
    return {o.s, o.x, o.y, o.heading, o.kappa, o.v, o.ax, o.u, o.t0, o.s0, o.e, o.dist2, o.seg, o.count,
            o.end_node, o.overspeed, o.t_end, o.t_loss, o.node_v, o.node_t};
}

// fill the queries' block (host) from q: a NULL row is 0, a NULL seg_hint -1
inline void query_pack(const rl_rjn_query& q, const QueryLayout& L, char* block) {
    std::memcpy(block + L.pose, q.pose_xy, L.Q * 16);
    if (L.K) std::memcpy(block + L.v0, q.v0, L.Q * 8);
    int32_t* row = (int32_t*)(block + L.row);
    int32_t* hint = (int32_t*)(block + L.hint);
    for (size_t k = 0; k < L.Q; ++k) {
        row[k] = q.row ? q.row[k] : 0;
        hint[k] = q.seg_hint ? q.seg_hint[k] : -1;
    }
}

// the same, and for a stop stage the targets: a NULL v_target is all 0.0
inline void query_pack(const rl_stp_query& q, const QueryLayout& L, char* block) {
    query_pack(q.rj, L, block);
    if (!L.stop) return;
    if (q.v_target) std::memcpy(block + L.v_target, q.v_target, L.Q * 8);
    else std::memset(block + L.v_target, 0, L.Q * 8);
    std::memcpy(block + L.stop_sample, q.stop_sample, L.Q * 4);
}

// the pointers and sizes of a launch of q on the blocks `in` and `out` (hz alone is the horizon
// kernel's); hz.src and cfg are the caller's
inline RjnParams query_pointers(const rl_rjn_query& q, const QueryLayout& L, char* in, char* out) {
    RjnParams r{};
    HznParams& h = r.hz;
    h.pose = (const double*)(in + L.pose);
    h.row = (const int32_t*)(in + L.row);
    h.hint = (const int32_t*)(in + L.hint);
    for (int c = 0; c < TRAJ_COLS; ++c) h.out[c] = (double*)(out + L.col[c]);
    for (int c = 0; c < HZN_LOC; ++c) h.loc[c] = (double*)(out + L.per[c]);
    h.seg = (int32_t*)(out + L.ints[0]);
    h.count = (int32_t*)(out + L.ints[1]);
    h.dt = q.dt;
    h.Q = q.Q; h.window = q.window; h.M_cap = q.M_cap;
    if (!L.K) return r;
    r.v0 = (const double*)(in + L.v0);
    for (int c = 0; c < RJN_SCAL; ++c) r.scal[c] = (double*)(out + L.per[HZN_LOC + c]);
    r.merge_node = (int32_t*)(out + L.ints[2]);
    r.overspeed = (int32_t*)(out + L.ints[3]);
    r.node_v = (double*)(out + L.nodes[0]);
    r.node_t = (double*)(out + L.nodes[1]);
    r.K_cap = q.K_cap;
    return r;
}

// the same, and for a stop stage the pointers of its extra arrays (rj alone is the rejoin kernel's)
inline StpParams query_pointers(const rl_stp_query& q, const QueryLayout& L, char* in, char* out) {
    StpParams s{};
    s.rj = query_pointers(q.rj, L, in, out);
    if (!L.stop) return s;
    s.v_target = (const double*)(in + L.v_target);
    s.stop_sample = (const int32_t*)(in + L.stop_sample);
    for (int c = 0; c < STP_SCAL; ++c) s.scal[c] = (double*)(out + L.sper[c]);
    s.reachable = (int32_t*)(out + L.sints[0]);
    s.brake_node = (int32_t*)(out + L.sints[1]);
    s.node_b = (double*)(out + L.node_b);
    return s;
}

// a retime stage's launch on the rejoin pointers r of its query: the pointers of its extra arrays
// in `out`, and the ceiling's cfg fields
inline RtmParams retime_pointers(const RjnParams& r, const rl_cfg& cfg, const QueryLayout& L, char* out) {
    RtmParams t{};
    t.rj = r;
    t.v_cap = cfg.v_cap_mps; t.a_lat_max = cfg.a_lat_max; t.kappa_eps = cfg.kappa_eps;
    t.v_excess = (double*)(out + L.rper[0]);
    t.feasible = (int32_t*)(out + L.rints[0]);
    t.bind_node = (int32_t*)(out + L.rints[1]);
    t.node_b = (double*)(out + L.rnodes[0]);
    t.node_c = (double*)(out + L.rnodes[1]);
    return t;
}

// copy a results' block (host) into the non-NULL fields of o; with node_v and node_t NULL only
// the head is read
inline void query_unpack(const char* block, const QueryLayout& L, const rl_rjn& o) {
    double* const col[TRAJ_COLS] = {o.s, o.x, o.y, o.heading, o.kappa, o.v, o.ax};
    double* const per[QRY_PER] = {o.u, o.t0, o.s0, o.e, o.dist2, o.t_merge, o.t_loss};
    int32_t* const ints[QRY_INTS] = {o.seg, o.count, o.merge_node, o.overspeed};
    double* const nodes[QRY_NODES] = {o.node_v, o.node_t};
    for (int c = 0; c < TRAJ_COLS; ++c)
        if (col[c]) std::memcpy(col[c], block + L.col[c], L.Q * L.M * 8);
    for (int c = 0; c < L.n_per; ++c)
        if (per[c]) std::memcpy(per[c], block + L.per[c], L.Q * 8);
    for (int c = 0; c < L.n_ints; ++c)
        if (ints[c]) std::memcpy(ints[c], block + L.ints[c], L.Q * 4);
    for (int c = 0; c < L.n_nodes; ++c)
        if (nodes[c]) std::memcpy(nodes[c], block + L.nodes[c], L.Q * (L.K + 1) * 8);
}

// the same, and for a stop stage its extra arrays; with node_v, node_t and node_b NULL only the
// head is read
inline void query_unpack(const char* block, const QueryLayout& L, const rl_stp& o) {
    query_unpack(block, L, as_rjn(o));
    if (!L.stop) return;
    double* const sper[STP_SCAL] = {o.s_stop, o.v_excess};
    int32_t* const sints[STP_INTS] = {o.reachable, o.brake_node};
    for (int c = 0; c < STP_SCAL; ++c)
        if (sper[c]) std::memcpy(sper[c], block + L.sper[c], L.Q * 8);
    for (int c = 0; c < STP_INTS; ++c)
        if (sints[c]) std::memcpy(sints[c], block + L.sints[c], L.Q * 4);
    if (o.node_b) std::memcpy(o.node_b, block + L.node_b, L.Q * (L.K + 1) * 8);
}
// whether a fetch into o needs the node arrays, which lie behind the head
inline bool query_wants_nodes(const rl_stp& o) { return o.node_v || o.node_t || o.node_b; }

// the same for a retime stage (L.retime set)
inline void query_unpack(const char* block, const QueryLayout& L, const rl_rtm& o) {
    query_unpack(block, L, as_rjn(o));
    int32_t* const rints[RTM_INTS] = {o.feasible, o.bind_node};
    double* const rnodes[RTM_NODES] = {o.node_b, o.node_c};
    if (o.v_excess) std::memcpy(o.v_excess, block + L.rper[0], L.Q * 8);
    for (int c = 0; c < RTM_INTS; ++c)
        if (rints[c]) std::memcpy(rints[c], block + L.rints[c], L.Q * 4);
    for (int c = 0; c < RTM_NODES; ++c)
        if (rnodes[c]) std::memcpy(rnodes[c], block + L.rnodes[c], L.Q * (L.K + 1) * 8);
}
inline bool query_wants_nodes(const rl_rtm& o) { return o.node_v || o.node_t || o.node_b || o.node_c; }

// the recover stage: its query's rejoin part in the stop forms, its layout, the rest of its
// queries' block (a NULL dir_xy leaves that part unread), its launch on the retime pointers t of
// its query and the bounds rows bnd (lo, hi, nx, ny on the device), and its results
inline QueryLayout recover_layout(const rl_rcv_query& q) {
    return recover_layout((size_t)q.rj.Q, (size_t)q.rj.M_cap, (size_t)q.rj.K_cap);
}
// (a fan stage's merge_len is [Q][C])
inline void recover_pack(const rl_rcv_query& q, const QueryLayout& L, char* block) {
    std::memcpy(block + L.merge_len, q.merge_len, L.Q * (L.C ? L.C : 1) * 8);
    if (q.dir_xy) std::memcpy(block + L.dir, q.dir_xy, L.Q * 16);
}
inline RcvParams recover_pointers(const RtmParams& t, const rl_rcv_query& q, const QueryLayout& L, const char* in, char* out,
                                  const double* const (&bnd)[4]) {
    RcvParams c{};
    c.rt = t;
    c.merge_len = (const double*)(in + L.merge_len);
    c.dir = q.dir_xy ? (const double*)(in + L.dir) : nullptr;
    c.lo = bnd[0]; c.hi = bnd[1]; c.nx = bnd[2]; c.ny = bnd[3];
    c.offset = (double*)(out + L.offset);
    for (int k = 0; k < RCV_SCAL; ++k) c.scal[k] = (double*)(out + L.cper[k]);
    c.clamped = (int32_t*)(out + L.cints[0]);
    c.offtrack = (int32_t*)(out + L.cints[1]);
    c.merge_node = (int32_t*)(out + L.cints[2]);
    c.node_o = (double*)(out + L.cnodes[0]);
    c.node_k = (double*)(out + L.cnodes[1]);
    return c;
}
// the retime part of a recover stage's results (rl_rcv begins with rl_rtm's fields)
inline rl_rtm as_rtm(const rl_rcv& o) {
    return {o.s, o.x, o.y, o.heading, o.kappa, o.v, o.ax, o.u, o.t0, o.s0, o.e, o.dist2, o.seg, o.count,
            o.end_node, o.overspeed, o.t_end, o.t_loss, o.node_v, o.node_t, o.feasible, o.bind_node, o.v_excess,
            o.node_b, o.node_c};
}
inline void query_unpack(const char* block, const QueryLayout& L, const rl_rcv& o) {
    query_unpack(block, L, as_rtm(o));
    double* const cper[RCV_SCAL] = {o.lo0, o.hi0};
    int32_t* const cints[RCV_INTS] = {o.clamped, o.offtrack, o.merge_node};
    double* const cnodes[RCV_NODES] = {o.node_o, o.node_k};
    if (o.offset) std::memcpy(o.offset, block + L.offset, L.Q * L.M * 8);
    for (int c = 0; c < RCV_SCAL; ++c)
        if (cper[c]) std::memcpy(cper[c], block + L.cper[c], L.Q * 8);
    for (int c = 0; c < RCV_INTS; ++c)
        if (cints[c]) std::memcpy(cints[c], block + L.cints[c], L.Q * 4);
    for (int c = 0; c < RCV_NODES; ++c)
        if (cnodes[c]) std::memcpy(cnodes[c], block + L.cnodes[c], L.Q * (L.K + 1) * 8);
}
inline bool query_wants_nodes(const rl_rcv& o) { return query_wants_nodes(as_rtm(o)) || o.node_o || o.node_k; }

// the fan stage: its layout, its launch on the recover pointers w of its query in the blocks in
// and out (recover_pointers') and the scratch block (device), and its results
inline QueryLayout fan_layout(size_t Q, size_t M, size_t K, size_t C) { return query_layout_of(Q, M, K, false, true, true, C); }
inline QueryLayout fan_layout(const rl_fan_query& q) {
    return fan_layout((size_t)q.rc.rj.Q, (size_t)q.rc.rj.M_cap, (size_t)q.rc.rj.K_cap, (size_t)q.n_cand);
}
inline FanParams fan_pointers(const RcvParams& w, const rl_cfg& cfg, const QueryLayout& L, char* out, char* scratch) {
    FanParams f{};
    f.win = w;
    f.C = (int32_t)L.C;
    f.best = (int32_t*)(out + L.best);
    for (int c = 0; c < FAN_TAB_INTS; ++c) f.tab_i[c] = (int32_t*)(out + L.tints[c]);
    for (int c = 0; c < FAN_TAB_SCAL; ++c) f.tab_d[c] = (double*)(out + L.tper[c]);
    // the candidates: the same query, the results of Q*C queries in the scratch block
    const QueryLayout S = recover_layout(L.Q * L.C, 0, L.K);
    rl_rjn_query sq{};
    sq.dt = w.rt.rj.hz.dt;
    sq.Q = (int32_t)(L.Q * L.C); sq.window = w.rt.rj.hz.window; sq.M_cap = w.rt.rj.hz.M_cap; sq.K_cap = w.rt.rj.K_cap;
    RjnParams r = query_pointers(sq, S, scratch, scratch);   // (the query pointers are replaced below)
    r.hz.src = w.rt.rj.hz.src;
    r.hz.pose = w.rt.rj.hz.pose; r.hz.row = w.rt.rj.hz.row; r.hz.hint = w.rt.rj.hz.hint;
    r.cfg = w.rt.rj.cfg;
    r.v0 = w.rt.rj.v0;
    RcvParams c{};
    c.rt = retime_pointers(r, cfg, S, scratch);
    c.merge_len = w.merge_len; c.dir = w.dir;
    c.lo = w.lo; c.hi = w.hi; c.nx = w.nx; c.ny = w.ny;
    c.offset = nullptr;                        // no ticks (S.M == 0: the columns have no bytes either)
    for (int k = 0; k < RCV_SCAL; ++k) c.scal[k] = (double*)(scratch + S.cper[k]);
    c.clamped = (int32_t*)(scratch + S.cints[0]);
    c.offtrack = (int32_t*)(scratch + S.cints[1]);
    c.merge_node = (int32_t*)(scratch + S.cints[2]);
    c.node_o = (double*)(scratch + S.cnodes[0]);
    c.node_k = (double*)(scratch + S.cnodes[1]);
    f.cand = c;
    for (int k = 0; k < FAN_XNODES; ++k) f.xnode[k] = (double*)(scratch + S.out_bytes + (size_t)k * (L.Q * L.C) * (L.K + 1) * 8);
    return f;
}
// the recover part of a fan stage's results (rl_fan begins with rl_rcv's fields)
inline rl_rcv as_rcv(const rl_fan& o) {
    return {o.s, o.x, o.y, o.heading, o.kappa, o.v, o.ax, o.u, o.t0, o.s0, o.e, o.dist2, o.seg, o.count,
            o.end_node, o.overspeed, o.t_end, o.t_loss, o.node_v, o.node_t, o.feasible, o.bind_node, o.v_excess,
            o.node_b, o.node_c, o.offset, o.clamped, o.offtrack, o.merge_node, o.lo0, o.hi0, o.node_o, o.node_k};
}
inline void query_unpack(const char* block, const QueryLayout& L, const rl_fan& o) {
    query_unpack(block, L, as_rcv(o));
    int32_t* const tints[FAN_TAB_INTS] = {o.cand_class, o.cand_feasible, o.cand_clamped, o.cand_merge_node, o.cand_overspeed,
                                          o.cand_bind_node};
    double* const tper[FAN_TAB_SCAL] = {o.cand_t_end, o.cand_t_loss, o.cand_v_excess};
    if (o.best) std::memcpy(o.best, block + L.best, L.Q * 4);
    for (int c = 0; c < FAN_TAB_INTS; ++c)
        if (tints[c]) std::memcpy(tints[c], block + L.tints[c], L.Q * L.C * 4);
    for (int c = 0; c < FAN_TAB_SCAL; ++c)
        if (tper[c]) std::memcpy(tper[c], block + L.tper[c], L.Q * L.C * 8);
}
inline bool query_wants_nodes(const rl_fan& o) { return query_wants_nodes(as_rcv(o)); }

}  // namespace rl
