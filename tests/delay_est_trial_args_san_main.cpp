// delay_est_trial_args_san_main.cpp -- the host side of
// acl_fleet_delay_est_trial_init / acl_fleet_delay_est_trial_batch
// (csrc/fleet_trial.hip: the argument checks) under host AddressSanitizer /
// UndefinedBehaviorSanitizer, without a GPU: every call below fails a check
// before any HIP call, or has nothing to fly. Built and run by
// scripts/delay_est_trial_args_san.sh (hipcc -Xarch_host
// -fsanitize=address,undefined on fleet_trial.hip's host code and this file;
// the entries fleet_trial.hip calls come from the built library and are never
// reached). Exit 0: every call returned what it must and no sanitizer report.
#include <stdio.h>
#include <string.h>

#include <string>

#include "aclswarm_amd.h"

static std::string g_err;

extern "C" acl_status_t acl__set_error(const char* msg) {
  g_err = msg;
  return ACL_ERR_INVALID_ARG;
}

static int g_fail = 0;
static acl_formations_t F;

// both entries: the batch under "acl_fleet_delay_est_trial_batch: ", the init
// under "acl_fleet_delay_est_trial_init: "
static void expect(const acl_fleet_delay_est_trial_args_t* y, const char* what, bool init = true) {
  for (int e = 0; e < (init ? 2 : 1); ++e) {
    g_err.clear();
    const acl_status_t r = e ? acl_fleet_delay_est_trial_init(y, F.n, nullptr)
                             : acl_fleet_delay_est_trial_batch(&F, y, nullptr);
    const char* who = e ? "acl_fleet_delay_est_trial_init" : "acl_fleet_delay_est_trial_batch";
    if (r != ACL_ERR_INVALID_ARG || g_err.find(what) == std::string::npos ||
        g_err.find(who) != 0) {
      printf("FAIL (%s): wanted \"%s\", got %d \"%s\"\n", who, what, (int)r, g_err.c_str());
      ++g_fail;
    }
  }
}

int main() {
  static char mem[64];  // never dereferenced: every call fails a check first
  memset(&F, 0, sizeof F);
  F.n = 13;
  F.n_formations = 1;
  F.adj = reinterpret_cast<decltype(F.adj)>(mem);
  acl_fleet_delay_est_trial_args_t y;
  memset(&y, 0, sizeof y);
  expect(nullptr, "null argument");
  acl_fleet_trial_args_t& a = y.est.lossy.delay.base;
  F.n = 129;
  expect(&y, "n out of range");
  F.n = 13;
  a.B = 1; a.K = 1; a.steps = 1;
  expect(&y, "ticks_per_step < 1");
  a.ticks_per_step = 10; a.queue_cap = 52;
  acl_default_trial_params(&a.tp);
  expect(&y, "max_lat out of range");
  y.est.lossy.delay.max_lat = 2;
  expect(&y, "track_every < 1");
  y.est.track_every = 2;
  for (int m : {-1, 8, 1 << 30}) {
    y.max_tlat = m;
    expect(&y, "max_tlat out of range [0, 7]");
  }
  y.max_tlat = 2;
  y.feed_loss = reinterpret_cast<const uint16_t*>(mem);
  expect(&y, "feed_loss is given and loc_n_missed is NULL");
  y.loc_n_missed = reinterpret_cast<int32_t*>(mem);
  y.enc = reinterpret_cast<acl_fleet_encounter_status_t*>(mem);
  expect(&y, "enc is given and enc_blind or enc_ghost is NULL");
  y.enc_blind = reinterpret_cast<int32_t*>(mem);
  expect(&y, "enc is given and enc_blind or enc_ghost is NULL");
  y.enc_ghost = reinterpret_cast<int32_t*>(mem);
  expect(&y, "required pointer is NULL");
  {
    // every pointer of the trial, in the struct's own order (fseq .. workspace)
    void** p = (void**)&a.fseq;
    void** end = (void**)&a.workspace;
    for (; p <= end; ++p) *p = mem;
  }
  a.workspace_bytes = acl_fleet_est_trial_workspace_bytes(13, 1, 52, 2);
  expect(&y, "lat is NULL");
  y.est.lossy.delay.lat = reinterpret_cast<const uint8_t*>(mem);
  expect(&y, "loss is NULL", false);  // (the init reads no loss matrix)
  y.est.lossy.link.loss = reinterpret_cast<const uint16_t*>(mem);
  y.est.lossy.link.seed = reinterpret_cast<const uint32_t*>(mem);
  y.est.lossy.link.n_lost = reinterpret_cast<int32_t*>(mem);
  expect(&y, "loc_stamp, loc_est, loc_round, loc_n_lost, loc_Pt or xst is NULL");
  y.est.loc_stamp = reinterpret_cast<int32_t*>(mem);
  y.est.loc_est = reinterpret_cast<double*>(mem);
  y.est.loc_round = reinterpret_cast<int32_t*>(mem);
  y.est.loc_n_lost = reinterpret_cast<int32_t*>(mem);
  y.est.loc_Pt = reinterpret_cast<uint16_t*>(mem);
  y.est.xst = reinterpret_cast<acl_fleet_est_episode_status_t*>(mem);
  expect(&y, "tlat is NULL");
  y.tlat = reinterpret_cast<const uint8_t*>(mem);
  expect(&y, "loc_workspace is NULL");
  y.loc_workspace = mem;
  const size_t need = acl_fleet_delay_localize_workspace_bytes(13, 1, 2);
  if (need != ((32 + 28 * 3 * 13 * 13 + 7) & ~(size_t)7)) {  // (padded to a multiple of 8)
    printf("FAIL: log bytes %zu\n", need);
    ++g_fail;
  }
  y.loc_workspace_bytes = need - 1;
  expect(&y, "loc_workspace_bytes is too small");
  y.loc_workspace_bytes = need;
  a.workspace_bytes -= 1;
  expect(&y, "workspace_bytes is too small (acl_fleet_est_trial_workspace_bytes)");
  if (sizeof(acl_fleet_encounter_status_t) != 32 || sizeof(acl_fleet_encounter_step_t) != 24) {
    printf("FAIL: record sizes\n");
    ++g_fail;
  }
  // nothing to fly: no pointer is looked at
  a.B = 0;
  if (acl_fleet_delay_est_trial_batch(&F, &y, nullptr) != ACL_OK ||
      acl_fleet_delay_est_trial_init(&y, 13, nullptr) != ACL_OK) {
    printf("FAIL: empty\n");
    ++g_fail;
  }
  printf(g_fail ? "%d failures\n" : "ok (%d failures)\n", g_fail);
  return g_fail ? 1 : 0;
}
