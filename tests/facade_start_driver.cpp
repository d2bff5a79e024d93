// facade_start_driver.cpp -- exercises the exchange-mode start of the C++
// facade (include/aclswarm_amd.hpp, Auctioneer::start with setBidExchange):
// fleets whose vehicles each hold their OWN assignment, and the latency of
// one start. Built by aclswarm_amd/build.py into
// aclswarm_amd/lib/libfacade_start_driver.so and loaded by
// tests/test_gpu_facade_start.py (and scripts/exchange_latency.py) via ctypes.
#include <chrono>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "aclswarm_amd.hpp"

namespace amd = acl::aclswarm::amd;

namespace {

struct Setup {
  amd::PtsMat p, q;
  amd::AdjMat adj;
  Setup(int n, const double* p_cm, const uint8_t* adj_cm, const double* q_cm)
      : p(n, 3), q(n, 3), adj(n, n) {
    std::copy(p_cm, p_cm + (size_t)3 * n, p.data());
    std::copy(q_cm, q_cm + (size_t)3 * n, q.data());
    std::copy(adj_cm, adj_cm + (size_t)n * n, adj.data());
  }
};

}  // namespace

// n exchange-mode vehicles; vehicle v gets its own assignment P_rows[v]
// (vehicle -> formation point, through setAssignmentIndices, which does not
// validate) and calls start(q) once. Inputs column-major as the facade takes
// them. Outputs per vehicle: sends (send-bid calls), iter (of the last one,
// -1 none), who / price [n][n] (that bid; untouched when none), status
// (lastStatus()), idle (isIdle()), err [n][err_len] (lastError()).
extern "C" int facade_start_fleet(int n, const double* p_cm, const uint8_t* adj_cm,
                                  const double* q_cm, const uint8_t* P_rows, int32_t* sends_out,
                                  int32_t* iter_out, int32_t* who_out, float* price_out,
                                  int32_t* status_out, uint8_t* idle_out, char* err_out,
                                  int err_len) {
  try {
    const Setup s(n, p_cm, adj_cm, q_cm);
    for (int v = 0; v < n; ++v) {
      amd::Auctioneer a((amd::vehidx_t)v, (uint8_t)n, false);
      a.setBidExchange(true);
      a.setFormation(s.p, s.adj);
      a.setAssignmentIndices(P_rows + (size_t)v * n);
      int sends = 0;
      int32_t last_iter = -1;
      a.setSendBidHandler([&](uint32_t, uint32_t iter, const amd::Auctioneer::BidConstPtr& b) {
        ++sends;
        last_iter = (int32_t)iter;
        for (int j = 0; j < n; ++j) {
          who_out[(size_t)v * n + j] = b->who[(size_t)j];
          price_out[(size_t)v * n + j] = b->price[(size_t)j];
        }
      });
      a.start(s.q);
      sends_out[v] = sends;
      iter_out[v] = last_iter;
      status_out[v] = (int32_t)a.lastStatus();
      idle_out[v] = a.isIdle() ? 1 : 0;
      std::snprintf(err_out + (size_t)v * err_len, (size_t)err_len, "%s", a.lastError().c_str());
    }
  } catch (const std::exception& e) {
    fprintf(stderr, "facade_start_fleet: %s\n", e.what());
    return 1;
  }
  return 0;
}

// One exchange-mode vehicle (vehid 0, the identity assignment): flush() and
// start(q), `warm` times unmeasured and then `reps` times with a host clock
// around each start() -- the call ends in the facade's own synchronise.
// us_out[reps]: microseconds per start.
extern "C" int facade_start_latency(int n, const double* p_cm, const uint8_t* adj_cm,
                                    const double* q_cm, int warm, int reps, double* us_out) {
  try {
    const Setup s(n, p_cm, adj_cm, q_cm);
    amd::Auctioneer a(0, (uint8_t)n, false);
    a.setBidExchange(true);
    a.setFormation(s.p, s.adj);
    for (int r = 0; r < warm + reps; ++r) {
      a.flush();
      const auto t0 = std::chrono::steady_clock::now();
      a.start(s.q);
      const auto t1 = std::chrono::steady_clock::now();
      if (a.lastStatus() != ACL_OK) throw std::runtime_error(a.lastError());
      if (r >= warm) us_out[r - warm] = std::chrono::duration<double, std::micro>(t1 - t0).count();
    }
  } catch (const std::exception& e) {
    fprintf(stderr, "facade_start_latency: %s\n", e.what());
    return 1;
  }
  return 0;
}
