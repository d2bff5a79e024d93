// delay_localize_args_san_main.cpp -- the host side of
// acl_fleet_delay_localize_batch (csrc/fleet_localize.hip: the argument checks
// and the workspace size) under host AddressSanitizer /
// UndefinedBehaviorSanitizer, without a GPU: every call below fails a check
// before any HIP call, or is an empty batch. Built and run by
// scripts/delay_localize_args_san.sh (hipcc -Xarch_host
// -fsanitize=address,undefined on fleet_localize.hip's host code and this
// file). Exit 0: every call returned what it must and no sanitizer report.
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

static void expect(const acl_formations_t* F, const acl_fleet_delay_localize_args_t* d,
                   const char* what) {
  g_err.clear();
  const acl_status_t r = acl_fleet_delay_localize_batch(F, d, nullptr);
  if (r != ACL_ERR_INVALID_ARG || g_err.find(what) == std::string::npos) {
    printf("FAIL: wanted \"%s\", got %d \"%s\"\n", what, (int)r, g_err.c_str());
    ++g_fail;
  }
}

int main() {
  static char mem[64];  // never dereferenced: every call fails a check first
  acl_formations_t F;
  memset(&F, 0, sizeof F);
  acl_fleet_delay_localize_args_t d;
  memset(&d, 0, sizeof d);
  acl_fleet_localize_args_t& a = d.base;
  expect(nullptr, &d, "null argument");
  expect(&F, nullptr, "null argument");
  F.n = 129;
  expect(&F, &d, "n out of range");
  F.n = 13;
  F.n_formations = 1;
  F.adj = reinterpret_cast<decltype(F.adj)>(mem);
  a.B = 1; a.rounds = 4; a.q_rounds = 2;
  expect(&F, &d, "q_rounds must be 1 or rounds");
  a.q_rounds = 4;
  for (int m : {-1, 8, 1 << 30}) {
    d.max_tlat = m;
    expect(&F, &d, "max_tlat out of range");
  }
  d.max_tlat = 7;
  expect(&F, &d, "required pointer is NULL");
  a.fidx = reinterpret_cast<const int32_t*>(mem);
  a.Pt = reinterpret_cast<const uint16_t*>(mem);
  a.stamp = reinterpret_cast<int32_t*>(mem);
  a.est = reinterpret_cast<double*>(mem);
  a.round = reinterpret_cast<int32_t*>(mem);
  a.status = reinterpret_cast<acl_fleet_localize_status_t*>(mem);
  expect(&F, &d, "q is NULL");
  a.q = reinterpret_cast<const double*>(mem);
  expect(&F, &d, "tlat is NULL");
  d.tlat = reinterpret_cast<const uint8_t*>(mem);
  expect(&F, &d, "workspace is NULL");
  d.workspace = mem;
  const size_t need = acl_fleet_delay_localize_workspace_bytes(13, 1, 7);
  if (need != 32 + 28 * 8 * 13 * 13) { printf("FAIL: workspace bytes %zu\n", need); ++g_fail; }
  d.workspace_bytes = need - 1;
  expect(&F, &d, "workspace_bytes is too small");
  d.workspace_bytes = need;
  d.feed_loss = reinterpret_cast<const uint16_t*>(mem);
  expect(&F, &d, "feed_loss is given and seed is NULL");
  a.seed = reinterpret_cast<const uint32_t*>(mem);
  expect(&F, &d, "feed_loss is given and n_missed is NULL");
  d.feed_loss = nullptr;
  expect(&F, &d, "seed is given and loss and feed_loss are NULL");
  // the size function at and past its limits (the largest is 128 * 128 * 28 * 8 * B bytes)
  if (acl_fleet_delay_localize_workspace_bytes(128, 0x7FFFFFFF, 7) !=
      (size_t)0x7FFFFFFF * (32 + (size_t)28 * 8 * 128 * 128)) { printf("FAIL: size\n"); ++g_fail; }
  for (int bad = 0; bad < 5; ++bad) {
    const int n = bad == 0 ? 0 : bad == 1 ? 129 : 13, B = bad == 2 ? 0 : 1;
    const int m = bad == 3 ? -1 : bad == 4 ? 8 : 0;
    if (acl_fleet_delay_localize_workspace_bytes(n, B, m) != 0) { printf("FAIL: size 0\n"); ++g_fail; }
  }
  a.B = 0;
  a.seed = nullptr;
  if (acl_fleet_delay_localize_batch(&F, &d, nullptr) != ACL_OK) { printf("FAIL: empty\n"); ++g_fail; }
  printf(g_fail ? "%d failures\n" : "ok (%d failures)\n", g_fail);
  return g_fail ? 1 : 0;
}
