// The process-wide stream pool.
//
// HIP streams outlive the sessions that use them: a session takes its streams from a per-process
// pool keyed by device and kind (plain, high priority, CU-masked with a given mask) and hands them
// back drained when it is destroyed.  A process that runs many sessions (the GPU test suite
// creates a few hundred) then creates its queues once instead of creating and destroying HIP
// queues -- CU-masked and priority ones included -- per session, the common factor of the
// intermittent stalls DESIGN.md 4.2 records (in session create / destroy).
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdlib>
#include <mutex>
#include <vector>
#include "mk_session.hpp"

using namespace mk;

static std::mutex g_pool_mu;
static StreamList g_pool;        // idle streams
static bool g_pool_closed = false;   // mk_shutdown ran: returned streams are destroyed, not pooled
static std::vector<int> g_pool_count;   // streams of the pool in existence per device (idle or owned)

static int& pool_count(int device) {   // g_pool_mu held
  if ((int)g_pool_count.size() <= device) g_pool_count.resize(device + 1, 0);
  return g_pool_count[device];
}

// Drain and destroy one stream on its device (the calling thread's device is restored).
static void stream_destroy(const PoolKey& k, hipStream_t st) {
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    --pool_count(k.device);
  }
  DeviceGuard dg;
  if (hipSetDevice(k.device) == hipSuccess) {
    (void)hipStreamSynchronize(st);
    wd_forget(st);
    (void)hipStreamDestroy(st);
  }
  (void)hipGetLastError();
}

// Every idle pooled stream is destroyed while the HIP runtime is still alive.  Before this, the
// pool's CU-masked and priority queues stayed alive into the runtime's own static teardown, which
// crashed in __cxa_finalize after a profiler had finalised (rocprofv3, profiles/r03/final3/prof32.log:
// the 32-subset shard's lookahead schedule is the path that creates CU-masked queues).  Registered
// with atexit at the first stream the pool creates -- after HIP initialised, so it runs before HIP's
// own exit handlers -- and called by the hosts' exit hooks (Python atexit, the R package's
// .onUnload / exit finalizer).  Idempotent; sessions still alive keep their streams, which are then
// destroyed when the session is.
extern "C" void mk_shutdown(void) {
  StreamList idle;
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    g_pool_closed = true;
    idle.swap(g_pool);
  }
  for (auto& o : idle) stream_destroy(o.first, o.second);
}
static void shutdown_at_exit() { mk_shutdown(); }

namespace mk {
// A stream of this kind on the current device (hipSetDevice(device) done by the caller), recorded
// in `owned` for the session's destructor.
hipError_t pool_stream(StreamList& owned, hipStream_t* st, int device, int kind, int prio,
                       const std::vector<uint32_t>& mask) {
  PoolKey k;
  k.device = device;
  k.kind = kind;
  k.prio = prio;
  k.mask = mask;
  StreamList evict;
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    for (size_t i = 0; i < g_pool.size(); ++i)
      if (g_pool[i].first == k) {
        *st = g_pool[i].second;
        g_pool.erase(g_pool.begin() + (long)i);
        owned.push_back({k, *st});
        return hipSuccess;
      }
    // No exact match: a session of another configuration (another shard size needs another CU mask).
    // Idle streams left by earlier sessions still hold hardware queues, and a new queue among them
    // ends up sharing one with another stream (serialising the split Cholesky's streams: 5,427 ->
    // 4,087 subset-iters/s at 32 subsets) -- well before GPU_MAX_HW_QUEUES streams exist: configs[1]
    // after the 32-subset shard in one process ran 15,045-15,356 -> 12,659-13,189 subset-iters/s,
    // configs[3]'s share 1,666-1,701 -> 1,092.  So the idle streams on the device go (oldest first)
    // until at most MK_POOL_CAP - 1 streams remain besides the new one (default 1: every idle one;
    // measured cap 8 / 5 / 1: 12,659 / 15,261 / 15,532 and 1,092 / 1,678 / 1,714,
    // profiles/r04/pool/).  Repeated sessions of one configuration still reuse their queues.
    static const int cap_env = env_int("MK_POOL_CAP", 1);
    int over = pool_count(device) + 1 - std::max(1, cap_env);
    for (size_t i = 0; i < g_pool.size() && over > 0;) {
      if (g_pool[i].first.device == device) {
        evict.push_back(g_pool[i]);
        g_pool.erase(g_pool.begin() + (long)i);
        --over;
      } else {
        ++i;
      }
    }
  }
  for (auto& o : evict) stream_destroy(o.first, o.second);
  hipError_t e;
  if (kind == SK_CUMASK) {
    // cuMaskSize = the device's CU count (as before the pool); the array is padded to that many
    // words so the runtime never reads past it, whichever unit it counts in (the words past the
    // CU count are ignored)
    const uint32_t size = (uint32_t)(mask.size() * 32);
    std::vector<uint32_t> padded(size, 0xffffffffu);
    for (size_t i = 0; i < mask.size(); ++i) padded[i] = mask[i];
    e = hipExtStreamCreateWithCUMask(st, size, padded.data());
  } else {
    e = kind == SK_PRIO ? hipStreamCreateWithPriority(st, hipStreamNonBlocking, prio)
                        : hipStreamCreateWithFlags(st, hipStreamNonBlocking);
  }
  if (e == hipSuccess) {
    owned.push_back({k, *st});
    {
      std::lock_guard<std::mutex> lk(g_pool_mu);
      ++pool_count(device);
    }
    static std::once_flag at_exit;
    std::call_once(at_exit, [] { std::atexit(shutdown_at_exit); });
  }
  return e;
}
void pool_return(StreamList& owned) {
  StreamList gone;
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    for (auto& o : owned) (g_pool_closed ? gone : g_pool).push_back(o);
  }
  owned.clear();
  for (auto& o : gone) stream_destroy(o.first, o.second);
}
hipError_t stream_acquire(int device, hipStream_t* st) {
  StreamList one;
  return pool_stream(one, st, device, SK_PLAIN);
}
void stream_release(int device, hipStream_t st) {
  StreamList one;
  PoolKey k;
  k.device = device;
  k.kind = SK_PLAIN;
  one.push_back({k, st});
  pool_return(one);
}
}  // namespace mk

// Hardware queues of this process's HIP runtime (mk_set_hw_queues; -1: GPU_MAX_HW_QUEUES as set in
// the environment, HIP's default 4 when unset).
static std::atomic<int> g_hw_queues{-1};
int mk::hw_queues() {
  const int n = g_hw_queues.load();
  return n >= 0 ? n : env_int("GPU_MAX_HW_QUEUES", 4);
}
extern "C" int mk_set_hw_queues(int32_t n) {
  g_hw_queues.store(n < 0 ? -1 : n);
  return 0;
}
