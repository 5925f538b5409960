// rl_query.h — the pose-query stages (horizon; rejoin, §3m; stop, §3n; retime, §3p;
// recover, §3q; fan, §3r) described once, for every host layer to read.  A stage is a QueryKind.
// kSlots names every array of the two packed blocks, in block order, with its element size, its
// extent and the kinds that have it; query_layout_of walks it with one cursor, so a slot a kind has
// not takes no room and moves nothing.  kKinds has, per kind, its name, the fields of its public
// results struct as (slot, offsetof) and the messages that fit no pattern; QueryKind itself, a
// kind's rl_plan_kernel_ms index and whether it reads the bounds stage are rl_stage_graph.h's, under
// stage_of(kind).  On these: one query form (QueryView), one query_pack, the *_pointers that fill
// the kernels' parameter structs, one query_unpack and one query_wants_nodes.  No HIP call: a host
// compiler builds it without a device (tests/query_layout_check.cpp).  Not part of the public ABI.
#pragma once
#include <cstddef>
#include <cstring>

#include "rl_abi.h"
#include "rl_stage_graph.h"
#include "rl_rejoin.h"
#include "rl_stop.h"
#include "rl_retime.h"
#include "rl_recover.h"
#include "rl_recover_fan.h"

namespace rl {

constexpr unsigned kbit(QueryKind k) { return 1u << (int)k; }
constexpr unsigned K_ALL = (1u << QUERY_KINDS) - 1;
constexpr unsigned K_FAN = kbit(QueryKind::Fan);
constexpr unsigned K_RCV = kbit(QueryKind::Recover) | K_FAN;       // the recover stage's arrays
constexpr unsigned K_RTM = kbit(QueryKind::Retime) | K_RCV;        // the retime stage's arrays
constexpr unsigned K_STP = kbit(QueryKind::Stop);
constexpr unsigned K_CAR = K_ALL & ~kbit(QueryKind::Horizon);      // from the car's speed: every stage but the horizon

// Every array of the two blocks, in block order.  The queries' block: S_POSE .. S_DIR.  The
// results' block: the head (always downloaded) S_S .. S_PAD_FAN: the columns [Q][M] in rl_hzn's
// order and offset, the doubles [Q], the candidates' doubles [Q][C], the ints [Q], best and the
// candidates' ints [Q][C]; then the node arrays [Q][K + 1], S_NODE_V .. S_NODE_K.  A stop stage's
// stop_node, t_stop and v_end lie in S_MERGE_NODE, S_T_MERGE and S_T_LOSS, a retime stage's
// end_node and t_end in S_MERGE_NODE and S_T_MERGE.  The two pad words per query keep the node
// arrays 8-byte aligned behind an odd number of ints.
enum Slot {
    S_POSE, S_V0, S_ROW, S_HINT, S_V_TARGET, S_STOP_SAMPLE, S_MERGE_LEN, S_DIR,
    S_S, S_X, S_Y, S_HEADING, S_KAPPA, S_V, S_AX, S_OFFSET,
    S_U, S_T0, S_S0, S_E, S_DIST2, S_T_MERGE, S_T_LOSS, S_S_STOP, S_V_EXCESS, S_LO0, S_HI0,
    S_CAND_T_END, S_CAND_T_LOSS, S_CAND_V_EXCESS,
    S_SEG, S_COUNT, S_MERGE_NODE, S_OVERSPEED, S_REACHABLE, S_BRAKE_NODE, S_FEASIBLE, S_BIND_NODE,
    S_CLAMPED, S_OFFTRACK, S_RCV_MERGE_NODE, S_PAD_RCV, S_BEST,
    S_CAND_CLASS, S_CAND_FEASIBLE, S_CAND_CLAMPED, S_CAND_MERGE_NODE, S_CAND_OVERSPEED, S_CAND_BIND_NODE, S_PAD_FAN,
    S_NODE_V, S_NODE_T, S_NODE_B, S_NODE_C, S_NODE_O, S_NODE_K,
    N_SLOTS,
    S_OUT_FIRST = S_S, S_NODE_FIRST = S_NODE_V       // where the results' block and its node side begin
};

// elements per slot: Q, Q*2, Q*M, Q*(K + 1), Q*C (C = 1 but for the fan stage)
enum Extent { X_Q, X_Q2, X_QM, X_QK, X_QC };

struct SlotInfo {
    const char* name;                                // the array's name where a results struct or a query has it
    unsigned char elem;                              // bytes per element
    Extent ext;
    unsigned kinds;                                  // the kinds whose blocks have it
};
constexpr SlotInfo kSlots[] = {
    {"pose", 8, X_Q2, K_ALL}, {"v0", 8, X_Q, K_CAR}, {"row", 4, X_Q, K_ALL}, {"hint", 4, X_Q, K_ALL},
    {"v_target", 8, X_Q, K_STP}, {"stop_sample", 4, X_Q, K_STP}, {"merge_len", 8, X_QC, K_RCV}, {"dir", 8, X_Q2, K_RCV},
    {"s", 8, X_QM, K_ALL}, {"x", 8, X_QM, K_ALL}, {"y", 8, X_QM, K_ALL}, {"heading", 8, X_QM, K_ALL},
    {"kappa", 8, X_QM, K_ALL}, {"v", 8, X_QM, K_ALL}, {"ax", 8, X_QM, K_ALL}, {"offset", 8, X_QM, K_RCV},
    {"u", 8, X_Q, K_ALL}, {"t0", 8, X_Q, K_ALL}, {"s0", 8, X_Q, K_ALL}, {"e", 8, X_Q, K_ALL}, {"dist2", 8, X_Q, K_ALL},
    {"t_merge", 8, X_Q, K_CAR}, {"t_loss", 8, X_Q, K_CAR}, {"s_stop", 8, X_Q, K_STP}, {"v_excess", 8, X_Q, K_STP | K_RTM},
    {"lo0", 8, X_Q, K_RCV}, {"hi0", 8, X_Q, K_RCV},
    {"cand_t_end", 8, X_QC, K_FAN}, {"cand_t_loss", 8, X_QC, K_FAN}, {"cand_v_excess", 8, X_QC, K_FAN},
    {"seg", 4, X_Q, K_ALL}, {"count", 4, X_Q, K_ALL}, {"merge_node", 4, X_Q, K_CAR}, {"overspeed", 4, X_Q, K_CAR},
    {"reachable", 4, X_Q, K_STP}, {"brake_node", 4, X_Q, K_STP}, {"feasible", 4, X_Q, K_RTM}, {"bind_node", 4, X_Q, K_RTM},
    {"clamped", 4, X_Q, K_RCV}, {"offtrack", 4, X_Q, K_RCV}, {"rcv_merge_node", 4, X_Q, K_RCV}, {"pad_rcv", 4, X_Q, K_RCV},
    {"best", 4, X_Q, K_FAN},
    {"cand_class", 4, X_QC, K_FAN}, {"cand_feasible", 4, X_QC, K_FAN}, {"cand_clamped", 4, X_QC, K_FAN},
    {"cand_merge_node", 4, X_QC, K_FAN}, {"cand_overspeed", 4, X_QC, K_FAN}, {"cand_bind_node", 4, X_QC, K_FAN},
    {"pad_fan", 4, X_Q, K_FAN},
    {"node_v", 8, X_QK, K_CAR}, {"node_t", 8, X_QK, K_CAR}, {"node_b", 8, X_QK, K_STP | K_RTM}, {"node_c", 8, X_QK, K_RTM},
    {"node_o", 8, X_QK, K_RCV}, {"node_k", 8, X_QK, K_RCV},
};
static_assert(sizeof(kSlots) / sizeof(kSlots[0]) == N_SLOTS, "one row of kSlots per slot");
// the kernels' parameter arrays index runs of slots
static_assert(S_AX - S_S + 1 == TRAJ_COLS && S_DIST2 - S_U + 1 == HZN_LOC && S_T_LOSS - S_T_MERGE + 1 == RJN_SCAL &&
                  S_V_EXCESS - S_S_STOP + 1 == STP_SCAL && S_HI0 - S_LO0 + 1 == RCV_SCAL &&
                  S_CAND_V_EXCESS - S_CAND_T_END + 1 == FAN_TAB_SCAL && S_CAND_BIND_NODE - S_CAND_CLASS + 1 == FAN_TAB_INTS,
              "the slot runs are the kernels' arrays");

// whether every 8-byte slot a kind has lies behind an even number of 4-byte elements per query (Q
// and C may be odd): the pad words are what makes it so
constexpr bool doubles_aligned(QueryKind k) {
    int words = 0;                                   // the 4-byte elements per query so far, C taken as 1
    for (int s = 0; s < N_SLOTS; ++s) {
        if (s == S_OUT_FIRST) words = 0;
        if (!(kSlots[s].kinds & kbit(k))) continue;
        if (kSlots[s].elem == 8 && words % 2) return false;
        if (kSlots[s].elem == 4) ++words;
    }
    return true;
}
static_assert(doubles_aligned(QueryKind::Horizon) && doubles_aligned(QueryKind::Rejoin) && doubles_aligned(QueryKind::Stop) &&
                  doubles_aligned(QueryKind::Retime) && doubles_aligned(QueryKind::Recover) && doubles_aligned(QueryKind::Fan),
              "the pads keep the doubles and the node arrays 8-byte aligned");

// ---------------------------------------------------------------- the kinds
// One pointer field of a kind's public results struct and the slot it is filled from.
struct FieldAt {
    Slot slot;
    size_t at;                                       // offsetof in the struct
};
#define RL_F(T, f, slot) {slot, offsetof(T, f)}
#define RL_HZN_FIELDS(T)                                                                                               \
    RL_F(T, s, S_S), RL_F(T, x, S_X), RL_F(T, y, S_Y), RL_F(T, heading, S_HEADING), RL_F(T, kappa, S_KAPPA), RL_F(T, v, S_V), \
        RL_F(T, ax, S_AX), RL_F(T, u, S_U), RL_F(T, t0, S_T0), RL_F(T, s0, S_S0), RL_F(T, e, S_E), RL_F(T, dist2, S_DIST2), \
        RL_F(T, seg, S_SEG), RL_F(T, count, S_COUNT)
// (node, ta, tb: the struct's names for what lies in S_MERGE_NODE, S_T_MERGE, S_T_LOSS)
#define RL_CAR_FIELDS(T, node, ta, tb)                                                                                 \
    RL_HZN_FIELDS(T), RL_F(T, node, S_MERGE_NODE), RL_F(T, overspeed, S_OVERSPEED), RL_F(T, ta, S_T_MERGE), RL_F(T, tb, S_T_LOSS), \
        RL_F(T, node_v, S_NODE_V), RL_F(T, node_t, S_NODE_T)
#define RL_RTM_FIELDS(T)                                                                                               \
    RL_CAR_FIELDS(T, end_node, t_end, t_loss), RL_F(T, feasible, S_FEASIBLE), RL_F(T, bind_node, S_BIND_NODE),         \
        RL_F(T, v_excess, S_V_EXCESS), RL_F(T, node_b, S_NODE_B), RL_F(T, node_c, S_NODE_C)
#define RL_RCV_FIELDS(T)                                                                                               \
    RL_RTM_FIELDS(T), RL_F(T, offset, S_OFFSET), RL_F(T, clamped, S_CLAMPED), RL_F(T, offtrack, S_OFFTRACK),           \
        RL_F(T, merge_node, S_RCV_MERGE_NODE), RL_F(T, lo0, S_LO0), RL_F(T, hi0, S_HI0), RL_F(T, node_o, S_NODE_O),    \
        RL_F(T, node_k, S_NODE_K)
constexpr FieldAt kHznFields[] = {RL_HZN_FIELDS(rl_hzn)};
constexpr FieldAt kRjnFields[] = {RL_CAR_FIELDS(rl_rjn, merge_node, t_merge, t_loss)};
constexpr FieldAt kStpFields[] = {RL_CAR_FIELDS(rl_stp, stop_node, t_stop, v_end), RL_F(rl_stp, reachable, S_REACHABLE),
                                  RL_F(rl_stp, brake_node, S_BRAKE_NODE), RL_F(rl_stp, s_stop, S_S_STOP),
                                  RL_F(rl_stp, v_excess, S_V_EXCESS), RL_F(rl_stp, node_b, S_NODE_B)};
constexpr FieldAt kRtmFields[] = {RL_RTM_FIELDS(rl_rtm)};
constexpr FieldAt kRcvFields[] = {RL_RCV_FIELDS(rl_rcv)};
constexpr FieldAt kFanFields[] = {RL_RCV_FIELDS(rl_fan), RL_F(rl_fan, best, S_BEST), RL_F(rl_fan, cand_class, S_CAND_CLASS),
                                  RL_F(rl_fan, cand_feasible, S_CAND_FEASIBLE), RL_F(rl_fan, cand_clamped, S_CAND_CLAMPED),
                                  RL_F(rl_fan, cand_merge_node, S_CAND_MERGE_NODE), RL_F(rl_fan, cand_overspeed, S_CAND_OVERSPEED),
                                  RL_F(rl_fan, cand_bind_node, S_CAND_BIND_NODE), RL_F(rl_fan, cand_t_end, S_CAND_T_END),
                                  RL_F(rl_fan, cand_t_loss, S_CAND_T_LOSS), RL_F(rl_fan, cand_v_excess, S_CAND_V_EXCESS)};
#undef RL_RCV_FIELDS
#undef RL_RTM_FIELDS
#undef RL_CAR_FIELDS
#undef RL_HZN_FIELDS
#undef RL_F

// whether a table names every pointer field of a struct of `bytes` bytes once, each from a slot of
// its own that the kind has
template <size_t n>
constexpr bool fields_cover(const FieldAt (&f)[n], size_t bytes, QueryKind k) {
    if (n * sizeof(void*) != bytes) return false;
    for (size_t i = 0; i < n; ++i) {
        if (f[i].at % sizeof(void*) || f[i].at >= bytes || f[i].slot < S_OUT_FIRST || !(kSlots[f[i].slot].kinds & kbit(k))) return false;
        for (size_t j = 0; j < i; ++j)
            if (f[j].at == f[i].at || f[j].slot == f[i].slot) return false;
    }
    return true;
}
static_assert(fields_cover(kHznFields, sizeof(rl_hzn), QueryKind::Horizon) && fields_cover(kRjnFields, sizeof(rl_rjn), QueryKind::Rejoin) &&
                  fields_cover(kStpFields, sizeof(rl_stp), QueryKind::Stop) && fields_cover(kRtmFields, sizeof(rl_rtm), QueryKind::Retime) &&
                  fields_cover(kRcvFields, sizeof(rl_rcv), QueryKind::Recover) && fields_cover(kFanFields, sizeof(rl_fan), QueryKind::Fan),
              "each kind's table covers sizeof(struct) / sizeof(void*) fields");

// A kind: its name in the entry points' names and messages, its results struct's fields, and the
// messages for a NULL query and for a fetch without a stage.
struct KindInfo {
    const char* name;
    const FieldAt* fields;
    int n_fields;
    const char* null_query;
    const char* fetch_none;
};
#define RL_FIELDS(t) t, (int)(sizeof(t) / sizeof(t[0]))
constexpr KindInfo kKinds[QUERY_KINDS] = {
    {"horizon", RL_FIELDS(kHznFields), "horizon: the query or its pose_xy is NULL",
     "rl_plan_fetch_horizon: no horizon stage since the plan's last run or trajectory stage"},
    {"rejoin", RL_FIELDS(kRjnFields), "rejoin: the query is NULL",
     "rl_plan_fetch_rejoin: no rejoin stage since the plan's last run or trajectory stage"},
    {"stop", RL_FIELDS(kStpFields), "stop: the query is NULL",
     "rl_plan_fetch_stop: no stop stage since the plan's last run or trajectory stage"},
    {"retime", RL_FIELDS(kRtmFields), "retime: the query is NULL",
     "rl_plan_fetch_retime: no retime stage since the plan's last run or trajectory stage"},
    {"recover", RL_FIELDS(kRcvFields), "recover: the query is NULL",
     "rl_plan_fetch_recover: no recover stage since the plan's last run, trajectory or bounds stage"},
    {"recover_fan", RL_FIELDS(kFanFields), "recover fan: the query is NULL",
     "rl_plan_fetch_recover_fan: no fan stage since the plan's last run, trajectory or bounds stage"},
};
#undef RL_FIELDS
inline const KindInfo& kind_info(QueryKind k) { return kKinds[(int)k]; }
constexpr bool reads_bounds(QueryKind k) { return stage_reads(stage_of(k), Stage::Bounds); }

// ---------------------------------------------------------------- the layout
// Where every slot lies for a stage of Q queries, M ticks, K nodes (0 for the horizon) and C
// candidates per query (0 but for the fan stage): off[] in its block, bytes[] 0 for a slot the kind
// has not.  in_bytes: the queries' block; head_bytes: the results' block up to the node arrays;
// out_bytes: all of it.  A fan stage's scratch block (scratch_bytes, on the device only) is the
// results' block of a recover stage of Q*C queries without ticks, then P.x, P.y, d', psi
// [Q*C][K + 1].
struct QueryLayout {
    size_t Q, M, K, C;
    QueryKind kind;
    size_t off[N_SLOTS], bytes[N_SLOTS];
    size_t in_bytes, head_bytes, out_bytes, scratch_bytes;
    bool has(Slot s) const { return (kSlots[s].kinds & kbit(kind)) != 0; }
};

inline QueryLayout query_layout_of(QueryKind kind, size_t Q, size_t M, size_t K, size_t C = 0) {
    QueryLayout L{};
    L.Q = Q; L.M = M; L.K = K; L.C = C;
    L.kind = kind;
    const size_t count[] = {Q, Q * 2, Q * M, Q * (K + 1), Q * (C ? C : 1)};   // by Extent
    size_t at = 0;                                   // the cursor
    for (int s = 0; s < N_SLOTS; ++s) {
        if (s == S_OUT_FIRST) { L.in_bytes = at; at = 0; }
        if (s == S_NODE_FIRST) L.head_bytes = at;
        L.off[s] = at;
        L.bytes[s] = L.has((Slot)s) ? count[kSlots[s].ext] * kSlots[s].elem : 0;
        at += L.bytes[s];
    }
    L.out_bytes = at;
    if (kind == QueryKind::Fan)
        L.scratch_bytes = query_layout_of(QueryKind::Recover, Q * C, 0, K).out_bytes + FAN_XNODES * (Q * C) * (K + 1) * 8;
    return L;
}

// ---------------------------------------------------------------- the queries
// Every kind's query in one form: the rejoin query (a horizon's without v0 and cfg, K_cap = 0) and
// what the later stages add, NULL / 0 where the kind has none.
struct QueryView {
    rl_rjn_query rj;
    const int32_t* stop_sample;                      // stop
    const double* v_target;
    const double* merge_len;                         // recover [Q], fan [Q][n_cand]
    const double* dir_xy;
    int32_t n_cand;                                  // fan
};
inline rl_rjn_query as_rjn(const rl_hzn_query& q) {
    return {q.pose_xy, q.row, q.seg_hint, q.Q, q.window, q.M_cap, 0, q.dt, nullptr, nullptr, 0, 0};
}
inline QueryView query_view(const rl_rjn_query& q) {
    QueryView v{};
    v.rj = q;
    return v;
}
inline QueryView query_view(const rl_hzn_query& q) { return query_view(as_rjn(q)); }
inline QueryView query_view(const rl_rtm_query& q) { return query_view(q.rj); }
inline QueryView query_view(const rl_stp_query& q) {
    QueryView v = query_view(q.rj);
    v.stop_sample = q.stop_sample;
    v.v_target = q.v_target;
    return v;
}
inline QueryView query_view(const rl_rcv_query& q) {
    QueryView v = query_view(q.rj);
    v.merge_len = q.merge_len;
    v.dir_xy = q.dir_xy;
    return v;
}
inline QueryView query_view(const rl_fan_query& q) {
    QueryView v = query_view(q.rc);
    v.n_cand = q.n_cand;
    return v;
}
inline QueryLayout query_layout_of(QueryKind kind, const QueryView& q) {
    return query_layout_of(kind, (size_t)q.rj.Q, (size_t)q.rj.M_cap, (size_t)q.rj.K_cap, (size_t)q.n_cand);
}

// fill the queries' block (host) from q: a NULL row is 0, a NULL seg_hint -1, a NULL v_target all
// 0.0; a NULL dir_xy leaves that part unwritten
inline void query_pack(const QueryView& q, const QueryLayout& L, char* block) {
    std::memcpy(block + L.off[S_POSE], q.rj.pose_xy, L.bytes[S_POSE]);
    if (L.has(S_V0)) std::memcpy(block + L.off[S_V0], q.rj.v0, L.bytes[S_V0]);
    int32_t* row = (int32_t*)(block + L.off[S_ROW]);
    int32_t* hint = (int32_t*)(block + L.off[S_HINT]);
    for (size_t k = 0; k < L.Q; ++k) {
        row[k] = q.rj.row ? q.rj.row[k] : 0;
        hint[k] = q.rj.seg_hint ? q.rj.seg_hint[k] : -1;
    }
    if (L.has(S_STOP_SAMPLE)) {
        if (q.v_target) std::memcpy(block + L.off[S_V_TARGET], q.v_target, L.bytes[S_V_TARGET]);
        else std::memset(block + L.off[S_V_TARGET], 0, L.bytes[S_V_TARGET]);
        std::memcpy(block + L.off[S_STOP_SAMPLE], q.stop_sample, L.bytes[S_STOP_SAMPLE]);
    }
    if (L.has(S_MERGE_LEN)) {
        std::memcpy(block + L.off[S_MERGE_LEN], q.merge_len, L.bytes[S_MERGE_LEN]);
        if (q.dir_xy) std::memcpy(block + L.off[S_DIR], q.dir_xy, L.bytes[S_DIR]);
    }
}

// ---------------------------------------------------------------- the launches' pointers
template <class T>
inline T* slot_ptr(const QueryLayout& L, char* block, int s) { return (T*)(block + L.off[s]); }

// the pointers and sizes of a launch of q on the blocks `in` and `out` (hz alone is the horizon
// kernel's, and all a horizon layout fills); hz.src and cfg are the caller's
inline RjnParams query_pointers(const rl_rjn_query& q, const QueryLayout& L, char* in, char* out) {
    RjnParams r{};
    HznParams& h = r.hz;
    h.pose = slot_ptr<const double>(L, in, S_POSE);
    h.row = slot_ptr<const int32_t>(L, in, S_ROW);
    h.hint = slot_ptr<const int32_t>(L, in, S_HINT);
    for (int c = 0; c < TRAJ_COLS; ++c) h.out[c] = slot_ptr<double>(L, out, S_S + c);
    for (int c = 0; c < HZN_LOC; ++c) h.loc[c] = slot_ptr<double>(L, out, S_U + c);
    h.seg = slot_ptr<int32_t>(L, out, S_SEG);
    h.count = slot_ptr<int32_t>(L, out, S_COUNT);
    h.dt = q.dt;
    h.Q = q.Q; h.window = q.window; h.M_cap = q.M_cap;
    if (L.kind == QueryKind::Horizon) return r;
    r.v0 = slot_ptr<const double>(L, in, S_V0);
    for (int c = 0; c < RJN_SCAL; ++c) r.scal[c] = slot_ptr<double>(L, out, S_T_MERGE + c);
    r.merge_node = slot_ptr<int32_t>(L, out, S_MERGE_NODE);
    r.overspeed = slot_ptr<int32_t>(L, out, S_OVERSPEED);
    r.node_v = slot_ptr<double>(L, out, S_NODE_V);
    r.node_t = slot_ptr<double>(L, out, S_NODE_T);
    r.K_cap = q.K_cap;
    return r;
}

// a stop stage's launch on the rejoin pointers r of its query: the pointers of its extra arrays
inline StpParams stop_pointers(const RjnParams& r, const QueryLayout& L, char* in, char* out) {
    StpParams s{};
    s.rj = r;
    s.v_target = slot_ptr<const double>(L, in, S_V_TARGET);
    s.stop_sample = slot_ptr<const int32_t>(L, in, S_STOP_SAMPLE);
    for (int c = 0; c < STP_SCAL; ++c) s.scal[c] = slot_ptr<double>(L, out, S_S_STOP + c);
    s.reachable = slot_ptr<int32_t>(L, out, S_REACHABLE);
    s.brake_node = slot_ptr<int32_t>(L, out, S_BRAKE_NODE);
    s.node_b = slot_ptr<double>(L, out, S_NODE_B);
    return s;
}

// a retime stage's launch on the rejoin pointers r of its query: the pointers of its extra arrays
// in `out`, and the ceiling's cfg fields
inline RtmParams retime_pointers(const RjnParams& r, const rl_cfg& cfg, const QueryLayout& L, char* out) {
    RtmParams t{};
    t.rj = r;
    t.v_cap = cfg.v_cap_mps; t.a_lat_max = cfg.a_lat_max; t.kappa_eps = cfg.kappa_eps;
    t.v_excess = slot_ptr<double>(L, out, S_V_EXCESS);
    t.feasible = slot_ptr<int32_t>(L, out, S_FEASIBLE);
    t.bind_node = slot_ptr<int32_t>(L, out, S_BIND_NODE);
    t.node_b = slot_ptr<double>(L, out, S_NODE_B);
    t.node_c = slot_ptr<double>(L, out, S_NODE_C);
    return t;
}

// a recover stage's launch on the retime pointers t of its query and the bounds rows bnd (lo, hi,
// nx, ny on the device); with_dir: the query has a dir_xy
inline RcvParams recover_pointers(const RtmParams& t, bool with_dir, const QueryLayout& L, char* in, char* out,
                                  const double* const (&bnd)[4]) {
    RcvParams c{};
    c.rt = t;
    c.merge_len = slot_ptr<const double>(L, in, S_MERGE_LEN);
    c.dir = with_dir ? slot_ptr<const double>(L, in, S_DIR) : nullptr;
    c.lo = bnd[0]; c.hi = bnd[1]; c.nx = bnd[2]; c.ny = bnd[3];
    c.offset = slot_ptr<double>(L, out, S_OFFSET);
    for (int k = 0; k < RCV_SCAL; ++k) c.scal[k] = slot_ptr<double>(L, out, S_LO0 + k);
    c.clamped = slot_ptr<int32_t>(L, out, S_CLAMPED);
    c.offtrack = slot_ptr<int32_t>(L, out, S_OFFTRACK);
    c.merge_node = slot_ptr<int32_t>(L, out, S_RCV_MERGE_NODE);
    c.node_o = slot_ptr<double>(L, out, S_NODE_O);
    c.node_k = slot_ptr<double>(L, out, S_NODE_K);
    return c;
}

// a fan stage's launch on the recover pointers w of its query in the results' block `out` and the
// scratch block (device)
inline FanParams fan_pointers(const RcvParams& w, const rl_cfg& cfg, const QueryLayout& L, char* out, char* scratch) {
    FanParams f{};
    f.win = w;
    f.C = (int32_t)L.C;
    f.best = slot_ptr<int32_t>(L, out, S_BEST);
    for (int c = 0; c < FAN_TAB_INTS; ++c) f.tab_i[c] = slot_ptr<int32_t>(L, out, S_CAND_CLASS + c);
    for (int c = 0; c < FAN_TAB_SCAL; ++c) f.tab_d[c] = slot_ptr<double>(L, out, S_CAND_T_END + c);
    // the candidates: a recover stage of Q*C queries without ticks whose results lie in the scratch
    // block; it reads the query's own arrays
    const QueryLayout S = query_layout_of(QueryKind::Recover, L.Q * L.C, 0, L.K);
    const HznParams& wh = w.rt.rj.hz;
    rl_rjn_query sq{};
    sq.dt = wh.dt;
    sq.Q = (int32_t)(L.Q * L.C); sq.window = wh.window; sq.M_cap = wh.M_cap; sq.K_cap = w.rt.rj.K_cap;
    RjnParams r = query_pointers(sq, S, scratch, scratch);
    r.hz.src = wh.src;
    r.hz.pose = wh.pose; r.hz.row = wh.row; r.hz.hint = wh.hint;
    r.cfg = w.rt.rj.cfg;
    r.v0 = w.rt.rj.v0;
    f.cand = recover_pointers(retime_pointers(r, cfg, S, scratch), false, S, scratch, scratch, {w.lo, w.hi, w.nx, w.ny});
    f.cand.merge_len = w.merge_len; f.cand.dir = w.dir;
    f.cand.offset = nullptr;                         // no ticks (S.M == 0: the columns have no bytes either)
    for (int k = 0; k < FAN_XNODES; ++k) f.xnode[k] = (double*)(scratch + S.out_bytes + (size_t)k * (L.Q * L.C) * (L.K + 1) * 8);
    return f;
}

// ---------------------------------------------------------------- the results
// the pointer a field of a results struct holds
inline void* field_ptr(const void* results, const FieldAt& f) {
    void* p;
    std::memcpy(&p, (const char*)results + f.at, sizeof p);
    return p;
}
// copy a results' block (host) into the non-NULL fields of o, L.kind's results struct; with its
// node arrays NULL only the head is read
inline void query_unpack(const char* block, const QueryLayout& L, const void* o) {
    const KindInfo& k = kind_info(L.kind);
    for (int i = 0; i < k.n_fields; ++i)
        if (void* dst = field_ptr(o, k.fields[i])) std::memcpy(dst, block + L.off[k.fields[i].slot], L.bytes[k.fields[i].slot]);
}
// whether a fetch into o, `kind`'s results struct, needs the node arrays, which lie behind the head
inline bool query_wants_nodes(QueryKind kind, const void* o) {
    const KindInfo& k = kind_info(kind);
    for (int i = 0; i < k.n_fields; ++i)
        if (k.fields[i].slot >= S_NODE_FIRST && field_ptr(o, k.fields[i])) return true;
    return false;
}

}  // namespace rl
