// rl_stage_graph.h — everything a plan (rl_host.h) can enqueue, described once: the run and the
// twelve stages that follow it, DESIGN §3t.  kStages has, per stage, its name, the stages whose
// results it reads and its rl_plan_kernel_ms indices.  From the reads come, on the host: what a
// stage waits for, what enqueuing it invalidates (StageSet::invalidate: the stage and, transitively,
// every stage that reads it), and which stages may still be reading what it is about to overwrite.
// The six pose-query kinds of rl_query.h lie in QueryKind's order, so stage_of and kind_of are
// arithmetic.  Plain C++, no include: a host compiler builds it alone (tests/stage_graph_check.cpp).
// Not part of the public ABI.
#pragma once

namespace rl {

enum class QueryKind { Horizon, Rejoin, Stop, Retime, Recover, Fan };
constexpr int QUERY_KINDS = 6;

enum class Stage { Run, Lap, Select, Trajectory, Bounds, HorizonBounds, Horizon, Rejoin, Stop, Retime, Recover, Fan, Rollouts };
constexpr int N_STAGES = 13;

constexpr Stage stage_of(QueryKind k) { return (Stage)((int)Stage::Horizon + (int)k); }
constexpr bool is_kind(Stage s) { return (int)s >= (int)Stage::Horizon && (int)s < (int)Stage::Horizon + QUERY_KINDS; }
constexpr QueryKind kind_of(Stage s) { return (QueryKind)((int)s - (int)Stage::Horizon); }   // of a stage that is_kind
static_assert(stage_of(QueryKind::Horizon) == Stage::Horizon && stage_of(QueryKind::Rejoin) == Stage::Rejoin &&
                  stage_of(QueryKind::Stop) == Stage::Stop && stage_of(QueryKind::Retime) == Stage::Retime &&
                  stage_of(QueryKind::Recover) == Stage::Recover && stage_of(QueryKind::Fan) == Stage::Fan &&
                  (int)Stage::Rollouts == N_STAGES - 1,
              "the kinds' stages lie in QueryKind's order");

constexpr unsigned sbit(Stage s) { return 1u << (int)s; }
constexpr unsigned R_RUN = sbit(Stage::Run);
constexpr unsigned R_TRAJ = R_RUN | sbit(Stage::Trajectory);
constexpr unsigned R_BND = R_TRAJ | sbit(Stage::Bounds);

// A stage: its name in the entry points' names, the stages it reads (a mask of sbit), and its
// rl_plan_kernel_ms indices ms_first .. ms_first + ms_count - 1 (include/rl_abi.h numbers them).
// The trajectory stage also uses the lap stage's rows and the selection's index, and a selection by
// lap the lap stage's lap: those are no reads here, because a later lap stage or selection leaves
// what was made from the old rows fetchable and only refuses new readers (rl_stages.cpp, traj_current).
struct StageInfo {
    const char* name;
    unsigned reads;
    int ms_first, ms_count;
};
constexpr StageInfo kStages[N_STAGES] = {
    {"run", 0, 0, 3},                  // the whole run and its two kernels
    {"lap", R_RUN, 4, 3},              // the stage, its preparation kernel, its evaluation kernel
    {"select", R_RUN, 3, 1},
    {"trajectory", R_RUN, 7, 1},
    {"bounds", R_TRAJ, 11, 1},
    {"horizon_bounds", R_RUN | sbit(Stage::Bounds) | sbit(Stage::Horizon), 12, 1},
    {"horizon", R_TRAJ, 8, 1},
    {"rejoin", R_TRAJ, 9, 1},
    {"stop", R_TRAJ, 10, 1},
    {"retime", R_TRAJ, 13, 1},
    {"recover", R_BND, 14, 1},
    {"recover_fan", R_BND, 15, 1},
    {"rollouts", R_BND, 16, 1},
};
constexpr const StageInfo& stage_info(Stage s) { return kStages[(int)s]; }
constexpr bool stage_reads(Stage s, Stage of) { return (kStages[(int)s].reads & sbit(of)) != 0; }

// the stage of a rl_plan_kernel_ms index, or -1
constexpr int stage_of_ms(int idx) {
    for (int s = 0; s < N_STAGES; ++s)
        if (idx >= kStages[s].ms_first && idx < kStages[s].ms_first + kStages[s].ms_count) return s;
    return -1;
}

// the stages that read `of`, directly or through another stage, `of` among them
constexpr unsigned stage_closure(Stage of) {
    unsigned m = sbit(of);
    for (unsigned before = 0; before != m;) {
        before = m;
        for (int s = 0; s < N_STAGES; ++s)
            if (kStages[s].reads & m) m |= 1u << s;
    }
    return m;
}

// Which stages of a plan hold results.  Enqueuing a stage starts with invalidate(stage).
struct StageSet {
    unsigned bits = 0;
    bool has(Stage s) const { return (bits & sbit(s)) != 0; }
    void set(Stage s) { bits |= sbit(s); }
    void invalidate(Stage s) { bits &= ~stage_closure(s); }
};

}  // namespace rl
