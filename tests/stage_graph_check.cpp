// stage_graph_check.cpp — csrc/rl_stage_graph.h against what the plan's entry points did before
// the table existed, written out here and not computed: what enqueuing each stage invalidates,
// which stage every rl_plan_kernel_ms index of include/rl_abi.h belongs to, and the stage <->
// QueryKind mapping.  A stand-alone host program (its own main, no HIP): tests/test_stage_graph_cpu.py
// builds and runs it.
#include <cstdio>
#include <cstring>

#include "rl_stage_graph.h"

using namespace rl;

static int failures = 0;
#define CHECK(cond, ...)                                                                                               \
    do {                                                                                                               \
        if (!(cond)) {                                                                                                 \
            ++failures;                                                                                                \
            std::printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond);                                                \
            std::printf(__VA_ARGS__);                                                                                  \
            std::printf("\n");                                                                                         \
        }                                                                                                              \
    } while (0)

constexpr Stage RUN = Stage::Run, LAP = Stage::Lap, SEL = Stage::Select, TRJ = Stage::Trajectory, BND = Stage::Bounds,
                HBD = Stage::HorizonBounds, HZN = Stage::Horizon, RJN = Stage::Rejoin, STP = Stage::Stop, RTM = Stage::Retime,
                RCV = Stage::Recover, FAN = Stage::Fan, RLL = Stage::Rollouts;
constexpr unsigned bits() { return 0; }
template <class... S>
constexpr unsigned bits(Stage s, S... more) { return 1u << (int)s | bits(more...); }

// enqueued -> the stages that no longer hold results (the enqueued one among them)
struct Row {
    Stage enqueued;
    const char* name;
    unsigned cleared;
};
static const Row kInvalidates[] = {
    {RUN, "run", bits(RUN, LAP, SEL, TRJ, BND, HBD, HZN, RJN, STP, RTM, RCV, FAN, RLL)},
    {LAP, "lap", bits(LAP)},
    {SEL, "select", bits(SEL)},
    {TRJ, "trajectory", bits(TRJ, BND, HBD, HZN, RJN, STP, RTM, RCV, FAN, RLL)},
    {BND, "bounds", bits(BND, HBD, RCV, FAN, RLL)},
    {HBD, "horizon_bounds", bits(HBD)},
    {HZN, "horizon", bits(HZN, HBD)},
    {RJN, "rejoin", bits(RJN)},
    {STP, "stop", bits(STP)},
    {RTM, "retime", bits(RTM)},
    {RCV, "recover", bits(RCV)},
    {FAN, "recover_fan", bits(FAN)},
    {RLL, "rollouts", bits(RLL)},
};

// rl_plan_kernel_ms index -> stage, as include/rl_abi.h lists them
static const Stage kMsStage[17] = {RUN, RUN, RUN, SEL, LAP, LAP, LAP, TRJ, HZN, RJN, STP, BND, HBD, RTM, RCV, FAN, RLL};

int main() {
    const unsigned all = (1u << N_STAGES) - 1;
    CHECK(sizeof(kInvalidates) / sizeof(kInvalidates[0]) == (size_t)N_STAGES, "one row per stage");
    for (const Row& r : kInvalidates) {
        CHECK(std::strcmp(stage_info(r.enqueued).name, r.name) == 0, "stage %d is named %s", (int)r.enqueued, stage_info(r.enqueued).name);
        StageSet v;
        for (int s = 0; s < N_STAGES; ++s) v.set((Stage)s);
        CHECK(v.bits == all, "set() of every stage");
        v.invalidate(r.enqueued);
        CHECK(v.bits == (all & ~r.cleared), "%s: left 0x%04x, the table says 0x%04x", r.name, v.bits, all & ~r.cleared);
        for (int s = 0; s < N_STAGES; ++s) CHECK(v.has((Stage)s) == !(r.cleared >> s & 1u), "%s: has(%s)", r.name, kStages[s].name);
        StageSet none;                               // invalidating on an empty set leaves it empty
        none.invalidate(r.enqueued);
        CHECK(none.bits == 0, "%s on an empty set", r.name);
        std::printf("%-14s clears 0x%04x\n", r.name, all & ~v.bits);
    }
    // a stage waits for what it reads: nothing reads itself, everything but the run reads the run
    for (int s = 0; s < N_STAGES; ++s) {
        CHECK(!stage_reads((Stage)s, (Stage)s), "%s reads itself", kStages[s].name);
        CHECK(stage_reads((Stage)s, RUN) == (s != (int)RUN), "%s and the run", kStages[s].name);
        CHECK((kStages[s].reads & ~all) == 0, "%s reads an unknown stage", kStages[s].name);
    }

    int seen[17] = {};
    for (int idx = 0; idx < 17; ++idx) {
        const int s = stage_of_ms(idx);
        CHECK(s == (int)kMsStage[idx], "kernel_ms %d belongs to stage %d, rl_abi.h says %s", idx, s, stage_info(kMsStage[idx]).name);
    }
    for (int s = 0; s < N_STAGES; ++s) {
        CHECK(kStages[s].ms_count >= 1, "%s has no kernel_ms index", kStages[s].name);
        for (int i = 0; i < kStages[s].ms_count; ++i) {
            const int idx = kStages[s].ms_first + i;
            CHECK(idx >= 0 && idx < 17, "%s: kernel_ms %d is out of range", kStages[s].name, idx);
            if (idx >= 0 && idx < 17) ++seen[idx];
        }
    }
    for (int idx = 0; idx < 17; ++idx) CHECK(seen[idx] == 1, "kernel_ms %d appears %d times", idx, seen[idx]);
    CHECK(stage_of_ms(-1) == -1 && stage_of_ms(17) == -1, "an index outside 0..16 has no stage");

    static const Stage kKindStage[QUERY_KINDS] = {HZN, RJN, STP, RTM, RCV, FAN};
    static const int kKindMs[QUERY_KINDS] = {8, 9, 10, 13, 14, 15};
    int kinds = 0;
    for (int k = 0; k < QUERY_KINDS; ++k) {
        const Stage s = stage_of((QueryKind)k);
        CHECK(s == kKindStage[k], "kind %d is stage %d", k, (int)s);
        CHECK(is_kind(s) && kind_of(s) == (QueryKind)k, "kind %d does not come back from its stage", k);
        CHECK(stage_info(s).ms_first == kKindMs[k] && stage_info(s).ms_count == 1, "kind %d: kernel_ms %d", k, stage_info(s).ms_first);
        CHECK(stage_reads(s, BND) == (k >= (int)QueryKind::Recover), "kind %d and the bounds stage", k);
    }
    for (int s = 0; s < N_STAGES; ++s)
        if (is_kind((Stage)s)) {
            ++kinds;
            CHECK(stage_of(kind_of((Stage)s)) == (Stage)s, "stage %s does not come back from its kind", kStages[s].name);
        }
    CHECK(kinds == QUERY_KINDS, "%d stages are kinds", kinds);

    std::printf(failures ? "%d checks failed\n" : "stage graph: all checks passed\n", failures);
    return failures ? 1 : 0;
}
