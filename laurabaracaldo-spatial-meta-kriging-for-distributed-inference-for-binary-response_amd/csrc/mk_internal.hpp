// Library-internal interface between the session (mk_api.hip, mk_pool.hip) and the multi-device
// driver (mk_multi.hip): a shard's quantile grids stay in HBM for the device-to-device combine.
// What the session's own sources share is in mk_session.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include "../../include/mk.h"

namespace mk {
struct ShardInfo {
  int device, S, P, q, n_test, tiled, pred_tile, n_kept;
  hipStream_t stream;
};
int host_error(int code, const char* msg);   // sets mk_last_error()
int session_info(const mk_session* s, ShardInfo* info);
// The grid kinds (mk_session_grids' `which`): [S][P][200] of the parameters; of a fused session
// [S][q n_test][200] of w.predict, or of p = pred_prob(draw) (needs x_test).
enum GridKind { GRID_PARAMETERS = 0, GRID_W = 1, GRID_P = 2 };
int session_grids(mk_session* s, GridKind kind, double* d_out);   // into HBM; returns after the stream is idle
// tiled: [S][q Tc][200]; d_out_p (optional): the p grids of the same replay
int session_tile_grids(mk_session* s, int t0, double* d_out, mk_outputs* o, double* d_out_p = nullptr);
// A plain non-blocking stream of the current device from libmk's stream pool, and its return
// (drained by the caller): the node driver's per-block streams live as long as the sessions' do.
// mk_maps.hip: MK_E_ARG naming the index of a non-finite threshold, or J when it is outside 0 .. MK_MAP_MAXT;
// touches no device.
int map_spec_check(const double* thresholds, int J);
// mk_pairs.hip: the checks of a pair spec that need no device -- the thresholds as above, and q >= 2.
int pair_spec_check(const mk_pair_spec* spec, int q);
hipError_t stream_acquire(int device, hipStream_t* st);
void stream_release(int device, hipStream_t st);

// Saves the calling thread's current device and restores it at scope exit.
struct DeviceGuard {
  int saved = -1;
  DeviceGuard() {
    if (hipGetDevice(&saved) != hipSuccess) {
      saved = -1;
      (void)hipGetLastError();
    }
  }
  ~DeviceGuard() {
    if (saved >= 0) (void)hipSetDevice(saved);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// Stall watchdog (mk_watch.hip; MK_WATCHDOG=<seconds>): wd_trace after every launch records the
// kernel's name for its stream and enqueues the progress-word store; ApiCall registers a C-ABI
// entry that may wait on the device, for the watchdog thread to report when it overruns.
bool wd_enabled();
void wd_trace(hipStream_t st, const char* name);
void wd_forget(hipStream_t st);
struct ApiCall {
  explicit ApiCall(const char* name);
  ~ApiCall();
  ApiCall(const ApiCall&) = delete;
  ApiCall& operator=(const ApiCall&) = delete;
  long id;
};
}  // namespace mk

// A kernel launch followed by its watchdog trace (a no-op unless the watchdog is on).
#define MK_LAUNCH(kernel, grid, block, lds, st, ...)                      \
  do {                                                                    \
    hipLaunchKernelGGL(kernel, grid, block, lds, st, __VA_ARGS__);        \
    ::mk::wd_trace(st, #kernel);                                          \
  } while (0)
