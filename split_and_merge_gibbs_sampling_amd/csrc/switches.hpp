// switches.hpp -- every HDPM_* environment switch of the engine: the one list of them (31), and the
// only place that calls getenv.  Host only.  A switch selects a path for A/B runs and diagnosis;
// the chain is the same with any of them (held to the oracle by tests/test_gpu_switches.py).  (The
// two other ways to steer the engine are the HDPM_DBG_* bits of hdpm_set_debug and the HDPM_OPT_*
// options of hdpm_set_option, include/hdpm.h.)
#pragma once
#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>

namespace hdpm::sw {

// How a value is read.  The first-character kinds are not the atoi kinds: "" and "abc" parse to 0,
// which turns a kOn switch off, but do not begin with '0', which leaves a kOnChr switch on.
enum Kind {
  kOn,      // on unless the value parses (atoi) to 0
  kOff,     // off unless the value parses (atoi) to 1
  kOnChr,   // on unless the value begins with '0'
  kOffChr,  // off unless the value begins with '1'
  kSet,     // on when the variable is set at all, to any value ("" and "0" too)
  kInt,     // integer (atoi), `def` when unset, clamped to [lo, hi]
  kIntOr,   // integer (atoi); outside [lo, hi] or not a multiple of `step` counts as unset: `def`
  kText,    // its own parser, below the list
};
// When a value is read: part of a switch's behaviour (a test of a kProcess switch needs a fresh
// process; a kLive one can be set after the library is loaded).
enum When {
  kProcess,  // once per process, at the first use of the path it steers
  kContext,  // at every hdpm_ctx_create (by the context, or by the host pool it creates)
  kLive,     // at every use
};
struct Switch {
  const char* name;
  Kind kind;
  When when;
  const char* meaning;
  int def = 0, lo = INT_MIN, hi = INT_MAX, step = 1;   // kInt / kIntOr
};
#define HDPM_SWITCH(id, ...) inline constexpr Switch id{"HDPM_" #id, __VA_ARGS__};
// diagnosis
HDPM_SWITCH(SEGV_TRACE, kSet, kProcess, "a host fault prints its stack's return addresses (read at library load)")
HDPM_SWITCH(SYNC_EACH, kOff, kProcess, "every kernel launch is synchronised and named on stderr with its status")
HDPM_SWITCH(WARM_SYNC, kOff, kProcess, "the same for the launches that warm the sweep's kernels up")
HDPM_SWITCH(WARM_MASK, kText, kProcess, "bit k clear skips the k-th warm-up launch (strtol, any base; default -1)")
HDPM_SWITCH(PHI_TRACE, kSet, kLive, "stderr: why a device update_phi was handed back; the stream priorities at create")
HDPM_SWITCH(PHI_TIMING, kSet, kLive, "phase marks of the fast device update, printed after a synchronous one")
// host pool, streams
HDPM_SWITCH(HOST_THREADS, kInt, kContext, "threads of the host pool; <= 0: the hardware's, at most 8")
HDPM_SWITCH(PIN_THREADS, kOn, kContext, "pool workers pinned to the cores of one L3 domain near the GPU")
HDPM_SWITCH(SPIN_US, kInt, kContext, "microseconds an idle pool worker spins before it sleeps", 2000, 0)
HDPM_SWITCH(STREAM_PRIO, kText, kContext, "first character 0: default stream priorities; 2: the sweep's stream low")
// update_phi
HDPM_SWITCH(PHI, kText, kContext, "host | device | device-general | (else) auto: HDPM_OPT_PHI_DEVICE's default")
HDPM_SWITCH(PHI_CHAIN, kOnChr, kProcess, "the next iteration's device update enqueued behind the current speculation")
HDPM_SWITCH(PHI2_GS, kInt, kProcess, "8, 16, 32 or 64 (checked by the caller): the fast update's group size")
HDPM_SWITCH(PHI2_GROUP_THREADS, kIntOr, kProcess, "threads of k_phi2_group's workgroups", 512, 128, 512, 64)
HDPM_SWITCH(PHI2_TREE_THREADS, kIntOr, kProcess, "threads of k_phi2_tree's workgroups; 0: by width", 0, 64, 1024, 64)
HDPM_SWITCH(PHI2_VALUES_WAVES, kIntOr, kProcess, "waves of k_phi2_values' workgroups; 0: by width", 0, 1, 16)
// pipeline of sweeps
HDPM_SWITCH(PIPE_AUTO, kOnChr, kProcess, "the device's own go for a sweep enqueued behind a fast device update")
HDPM_SWITCH(PIPE_EARLY, kOnChr, kProcess, "the host's early conditional go at the join of the speculated update")
HDPM_SWITCH(RES_WORD, kOnChr, kProcess, "a pipelined round's end taken from its sequence word; 0 keeps the event")
// sweep
HDPM_SWITCH(DENSE_LIST, kOn, kProcess, "launches that expect most points uncertain list every point")
HDPM_SWITCH(DENSE_DIRECT, kOn, kProcess, "dense launches skip the prepass; 0: they still run it")
HDPM_SWITCH(FPG_MIN, kInt, kProcess, "expected listed points from which launches take k_resolve_fpg", 1024, 1)
HDPM_SWITCH(FP_UNSETTLED_UNIF, kOn, kProcess, "the uniform's certification kept after an unsettled launch; 0: margins")
HDPM_SWITCH(LAT_BOUND, kOn, kProcess, "far latents kept as head bounds by the level-table exact rows; 0: all exact")
HDPM_SWITCH(LV_SPEC, kOn, kProcess, "snapshot draws behind the level-table exact rows (k_snap_draws)")
HDPM_SWITCH(MASS_STATIC, kInt, kProcess, "k_exact_rows_mass: nonzero walks the batches in a fixed order (no claims)")
HDPM_SWITCH(WIDE_WGS, kIntOr, kProcess, "workgroups of k_prepass_wide per CU; 0: by occupancy", 0, 1, 32)
HDPM_SWITCH(WIDE_CLAIM, kInt, kProcess, "k_prepass_wide: nonzero claims chunks from a counter")
// random stream, split-merge
HDPM_SWITCH(MT_WORKGROUPS, kIntOr, kProcess, "workgroups of the device stream generator", 256, 2, 4096)
HDPM_SWITCH(SM_CHAIN, kOffChr, kContext, "1: HDPM_OPT_SM_CHAIN starts at 1 (the restricted sampler as a device chain)")
HDPM_SWITCH(SM_WIDE, kOnChr, kProcess, "restricted scans on many CUs (k_sm_scan_wide); 0: one workgroup only")
#undef HDPM_SWITCH

// The value of switch s for the variable's text e (nullptr: unset).  Flags give 0 / 1.
inline int parse(const Switch& s, const char* e) {
  const int v = e ? std::atoi(e) : s.def;
  switch (s.kind) {
    case kOn: return !(e && v == 0);
    case kOff: return e && v == 1;
    case kOnChr: return !(e && e[0] == '0');
    case kOffChr: return e && e[0] == '1';
    case kInt: return e ? std::min(s.hi, std::max(s.lo, v)) : s.def;
    case kIntOr: return v >= s.lo && v <= s.hi && v % s.step == 0 ? v : s.def;
    default: return e != nullptr;   // kSet, kText
  }
}
// A switch's value, read when its entry says: a kProcess switch at its first get and never again,
// the others at every get (a kContext switch is one whose gets are on hdpm_ctx_create's path).
template <const Switch& S>
inline int get() {
  static_assert(S.kind != kText, "text switches have their own accessor");
  if constexpr (S.when == kProcess) {
    static const int v = parse(S, std::getenv(S.name));
    return v;
  }
  return parse(S, std::getenv(S.name));
}
// HDPM_PHI: the HDPM_OPT_PHI_DEVICE value a context starts with.
inline int phi_mode() {
  const char* e = std::getenv(PHI.name);
  if (!e) return 3;
  return !std::strcmp(e, "host") ? 0 : !std::strcmp(e, "device") ? 1 : !std::strcmp(e, "device-general") ? 2 : 3;
}
// HDPM_STREAM_PRIO: its first character, 0 when unset or empty.
inline char stream_prio() {
  const char* e = std::getenv(STREAM_PRIO.name);
  return e ? e[0] : 0;
}
inline int warm_mask() {
  static const char* const e = std::getenv(WARM_MASK.name);
  static const int v = e ? (int)std::strtol(e, nullptr, 0) : -1;
  return v;
}

}  // namespace hdpm::sw
