// CPU test of the environment-switch table (csrc/switches.hpp): how each kind of switch reads
// an unset variable, "0", "1", "2", "" and "abc", the defaults and ranges of the integer ones, the
// text switches' own parsers, and when a value is read: a once-per-process switch keeps its
// first value after setenv, a per-context or live one follows the environment.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>

#include "../../split_and_merge_gibbs_sampling_amd/csrc/switches.hpp"

namespace sw = hdpm::sw;

static int fails = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);      \
      ++fails;                                                     \
    }                                                              \
  } while (0)

// the six values every kind is asked about: unset, "0", "1", "2", "", "abc"
static const char* const kTexts[6] = {nullptr, "0", "1", "2", "", "abc"};
static void expect(const sw::Switch& s, sw::Kind kind, const int (&want)[6]) {
  CHECK(s.kind == kind);
  for (int q = 0; q < 6; ++q) {
    const int got = sw::parse(s, kTexts[q]);
    if (got != want[q]) {
      std::printf("FAIL %s = %s: %d, expected %d\n", s.name, kTexts[q] ? kTexts[q] : "(unset)", got, want[q]);
      ++fails;
    }
  }
}
static int of(const sw::Switch& s, const char* text) { return sw::parse(s, text); }

int main() {
  // the list: 31 switches, distinct HDPM_ names, a meaning each
  {
    const sw::Switch* const all[] = {
        &sw::SEGV_TRACE, &sw::SYNC_EACH, &sw::WARM_SYNC, &sw::WARM_MASK, &sw::PHI_TRACE, &sw::PHI_TIMING,
        &sw::HOST_THREADS, &sw::PIN_THREADS, &sw::SPIN_US, &sw::STREAM_PRIO, &sw::PHI, &sw::PHI_CHAIN, &sw::PHI2_GS,
        &sw::PHI2_GROUP_THREADS, &sw::PHI2_TREE_THREADS, &sw::PHI2_VALUES_WAVES, &sw::PIPE_AUTO, &sw::PIPE_EARLY,
        &sw::RES_WORD, &sw::DENSE_LIST, &sw::DENSE_DIRECT, &sw::FPG_MIN, &sw::FP_UNSETTLED_UNIF, &sw::LAT_BOUND,
        &sw::LV_SPEC, &sw::MASS_STATIC, &sw::WIDE_WGS, &sw::WIDE_CLAIM, &sw::MT_WORKGROUPS, &sw::SM_CHAIN, &sw::SM_WIDE};
    std::set<std::string> names;
    for (const sw::Switch* s : all) {
      CHECK(std::strncmp(s->name, "HDPM_", 5) == 0);
      CHECK(s->meaning && s->meaning[0]);
      CHECK(s->lo <= s->hi && s->step >= 1);
      names.insert(s->name);
    }
    CHECK(names.size() == 31 && sizeof(all) / sizeof(all[0]) == 31);
    CHECK(std::strcmp(sw::FPG_MIN.name, "HDPM_FPG_MIN") == 0);
  }
  // flags, by kind                                    unset "0" "1" "2" ""  "abc"
  expect(sw::DENSE_LIST, sw::kOn, {1, 0, 1, 1, 0, 0});
  expect(sw::PIN_THREADS, sw::kOn, {1, 0, 1, 1, 0, 0});
  expect(sw::SYNC_EACH, sw::kOff, {0, 0, 1, 0, 0, 0});
  expect(sw::RES_WORD, sw::kOnChr, {1, 0, 1, 1, 1, 1});
  expect(sw::PIPE_EARLY, sw::kOnChr, {1, 0, 1, 1, 1, 1});
  expect(sw::SM_CHAIN, sw::kOffChr, {0, 0, 1, 0, 0, 0});
  expect(sw::PHI_TRACE, sw::kSet, {0, 1, 1, 1, 1, 1});
  // (where the first-character kinds and the atoi kinds part)
  CHECK(of(sw::SM_CHAIN, "10") == 1 && of(sw::SYNC_EACH, "10") == 0);
  CHECK(of(sw::RES_WORD, " 0") == 1 && of(sw::DENSE_LIST, " 0") == 0);
  CHECK(of(sw::RES_WORD, "01") == 0 && of(sw::DENSE_LIST, "01") == 1);
  // integers: default when unset, clamped
  expect(sw::FPG_MIN, sw::kInt, {1024, 1, 1, 2, 1, 1});       // max(1, .)
  CHECK(of(sw::FPG_MIN, "-5") == 1 && of(sw::FPG_MIN, "300") == 300);
  expect(sw::SPIN_US, sw::kInt, {2000, 0, 1, 2, 0, 0});       // max(0, .)
  CHECK(of(sw::SPIN_US, "-5") == 0 && of(sw::SPIN_US, "50000") == 50000);
  expect(sw::HOST_THREADS, sw::kInt, {0, 0, 1, 2, 0, 0});     // (the pool takes <= 0 as automatic)
  CHECK(of(sw::HOST_THREADS, "-3") == -3 && of(sw::HOST_THREADS, "12") == 12);
  expect(sw::WIDE_CLAIM, sw::kInt, {0, 0, 1, 2, 0, 0});
  // integers: a value outside the range counts as unset
  expect(sw::MT_WORKGROUPS, sw::kIntOr, {256, 256, 256, 2, 256, 256});
  CHECK(of(sw::MT_WORKGROUPS, "4096") == 4096 && of(sw::MT_WORKGROUPS, "4097") == 256 &&
        of(sw::MT_WORKGROUPS, "128") == 128);
  expect(sw::PHI2_GROUP_THREADS, sw::kIntOr, {512, 512, 512, 512, 512, 512});
  CHECK(of(sw::PHI2_GROUP_THREADS, "128") == 128 && of(sw::PHI2_GROUP_THREADS, "256") == 256 &&
        of(sw::PHI2_GROUP_THREADS, "200") == 512 && of(sw::PHI2_GROUP_THREADS, "64") == 512 &&
        of(sw::PHI2_GROUP_THREADS, "576") == 512);
  expect(sw::PHI2_TREE_THREADS, sw::kIntOr, {0, 0, 0, 0, 0, 0});
  CHECK(of(sw::PHI2_TREE_THREADS, "64") == 64 && of(sw::PHI2_TREE_THREADS, "1024") == 1024 &&
        of(sw::PHI2_TREE_THREADS, "100") == 0 && of(sw::PHI2_TREE_THREADS, "1088") == 0);
  expect(sw::PHI2_VALUES_WAVES, sw::kIntOr, {0, 0, 1, 2, 0, 0});
  CHECK(of(sw::PHI2_VALUES_WAVES, "16") == 16 && of(sw::PHI2_VALUES_WAVES, "17") == 0);
  expect(sw::WIDE_WGS, sw::kIntOr, {0, 0, 1, 2, 0, 0});
  CHECK(of(sw::WIDE_WGS, "32") == 32 && of(sw::WIDE_WGS, "33") == 0 && of(sw::WIDE_WGS, "-1") == 0);

  // when a value is read.  Once per process: the first get decides
  setenv("HDPM_DENSE_LIST", "0", 1);
  CHECK(sw::get<sw::DENSE_LIST>() == 0);
  setenv("HDPM_DENSE_LIST", "1", 1);
  CHECK(sw::get<sw::DENSE_LIST>() == 0);
  unsetenv("HDPM_DENSE_LIST");
  CHECK(sw::get<sw::DENSE_LIST>() == 0);
  unsetenv("HDPM_FPG_MIN");
  CHECK(sw::get<sw::FPG_MIN>() == 1024);
  setenv("HDPM_FPG_MIN", "7", 1);
  CHECK(sw::get<sw::FPG_MIN>() == 1024);
  // (a switch not yet used is still open: it is read at its own first use, not at another's)
  setenv("HDPM_RES_WORD", "0", 1);
  CHECK(sw::get<sw::RES_WORD>() == 0);
  // live: every get reads the environment
  unsetenv("HDPM_PHI_TRACE");
  CHECK(sw::get<sw::PHI_TRACE>() == 0);
  setenv("HDPM_PHI_TRACE", "1", 1);
  CHECK(sw::get<sw::PHI_TRACE>() == 1);
  unsetenv("HDPM_PHI_TRACE");
  CHECK(sw::get<sw::PHI_TRACE>() == 0);
  CHECK(sw::PHI_TRACE.when == sw::kLive && sw::PHI_TIMING.when == sw::kLive);
  // per context: read at every create
  unsetenv("HDPM_SPIN_US");
  CHECK(sw::get<sw::SPIN_US>() == 2000);
  setenv("HDPM_SPIN_US", "-4", 1);
  CHECK(sw::get<sw::SPIN_US>() == 0);
  setenv("HDPM_SPIN_US", "150", 1);
  CHECK(sw::get<sw::SPIN_US>() == 150);
  CHECK(sw::SPIN_US.when == sw::kContext);

  // the text switches
  unsetenv("HDPM_PHI");
  CHECK(sw::phi_mode() == 3);
  const char* const modes[] = {"host", "device", "device-general", "auto", "", "abc", "Device"};
  const int mode_of[] = {0, 1, 2, 3, 3, 3, 3};
  for (int q = 0; q < 7; ++q) {
    setenv("HDPM_PHI", modes[q], 1);
    CHECK(sw::phi_mode() == mode_of[q]);
  }
  unsetenv("HDPM_STREAM_PRIO");
  CHECK(sw::stream_prio() == 0);
  setenv("HDPM_STREAM_PRIO", "0", 1);
  CHECK(sw::stream_prio() == '0');
  setenv("HDPM_STREAM_PRIO", "2", 1);
  CHECK(sw::stream_prio() == '2');
  setenv("HDPM_STREAM_PRIO", "", 1);
  CHECK(sw::stream_prio() == 0);
  setenv("HDPM_WARM_MASK", "0x5", 1);          // strtol, any base; once per process
  CHECK(sw::warm_mask() == 5);
  setenv("HDPM_WARM_MASK", "7", 1);
  CHECK(sw::warm_mask() == 5);

  if (fails) return 1;
  std::printf("switches ok\n");
  return 0;
}
