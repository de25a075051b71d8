// feinsum_hip.hip -- C ABI of libfeinsum_hip.so (see include/feinsum_hip.h).
// gfx950 only.  Host side: argument validation, kernel-variant dispatch (the
// build's replacement for feinsum's transform archive lookup,
// sql_utils.py:247-294) and asynchronous launches on the caller's stream.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <mutex>
#include <string>
#include <tuple>
#include <type_traits>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/feinsum_hip.h"
#include "fe_common.h"
#include "fe_adjoint.h"
#include "fe_elemop.h"
#include "fe_weightedop.h"
#include "fe_weightgrad.h"
#include "fe_opgrad.h"
#include "fe_contract.h"
#include "fe_div.h"
#include "fe_einsum.h"
#include "fe_reduce.h"
#include "fe_facemass.h"
#include "fe_fused.h"
#include "fe_generic.h"
#include "fe_grad.h"
#include "fe_grad_f32.h"
#include "fe_div_f32.h"
#include "fe_facemass_f32.h"
#include "fe_tiled.h"
#include "fe_mixed.h"
#include "fe_orders.h"

static_assert(FE_FM_J_FE == 1 && FE_FM_R_IFJ == 2 && FE_FM_R_T == 4, "the layout bits fe::FmLayout decodes");

namespace {

thread_local char g_err[512] = "";

// Counts the FE_EHIP returns of this process: after a HIP error a launch may not have run to completion, and a dynamic launch
// that stopped half way leaves tickets in its counter group (later launches through that group would skip tiles).  The first
// dynamic launch of every stream after such a return verifies its group once (tail_slot below).
std::atomic<unsigned> g_hip_error_epoch{0};

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    if (code == FE_EHIP) g_hip_error_epoch.fetch_add(1, std::memory_order_relaxed);
    return code;
}

// (a failed call is reported once: HIP's per-thread "last error" is cleared here, or the launch after it -- which ends with
//  FE_HIP_CHECK(hipGetLastError()) -- would report the same, already handled error again)
#define FE_HIP_CHECK(expr)                                                             \
    do {                                                                               \
        hipError_t _e = (expr);                                                        \
        if (_e != hipSuccess) {                                                        \
            (void)hipGetLastError();                                                   \
            return fail(FE_EHIP, "%s failed: %s", #expr, hipGetErrorString(_e));       \
        }                                                                              \
    } while (0)

// Persistent-style grid: enough blocks to fill every CU at the kernel's
// residency (2 blocks of 256 threads per CU), capped by the work available.
std::atomic<int> g_cu_limit{[] { const char* e = getenv("FEINSUM_CU_LIMIT"); return e ? atoi(e) : 0; }()};
int device_cu_count() {
    // fe_set_cu_limit / FEINSUM_CU_LIMIT: size the persistent grids as if the device had fewer CUs (a CPX / QPX partition
    // of MI355X reports 32 / 64) -- a test hook for the small-grid paths, and a way to leave part of the device to others
    const int limit = g_cu_limit.load(std::memory_order_relaxed);
    static int cus[64];
    static std::once_flag once[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return limit > 0 && limit < 256 ? limit : 256;
    std::call_once(once[dev], [dev] {
        hipDeviceProp_t p;
        cus[dev] = (hipGetDeviceProperties(&p, dev) == hipSuccess && p.multiProcessorCount > 0)
                       ? p.multiProcessorCount
                       : 256;
    });
    return limit > 0 && limit < cus[dev] ? limit : cus[dev];
}

// Resources of every kernel configured so far in this process (fe_kernel_resources).
std::mutex g_resources_mutex;
std::string g_resources;

// Once per (kernel, device): raise the dynamic-LDS limit, then check that the compiled kernel really
// has the residency its launch geometry assumes.  The persistent grids are sized as
// blocks_per_cu x #CUs; if a compiler change pushed the kernel over a register step (> 256 VGPRs
// at two blocks of four waves per CU) the grid's second half would silently queue behind the
// first and every test would still pass at half the speed.
template <typename K>
int configure_kernel(K kernel, const char* what, int lds_bytes, int threads, int blocks_per_cu) {
    const void* fn = reinterpret_cast<const void*>(kernel);
    FE_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
    int resident = 0;
    FE_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&resident, fn, threads, (size_t)lds_bytes));
    hipFuncAttributes attr;
    FE_HIP_CHECK(hipFuncGetAttributes(&attr, fn));
    {
        char line[256];
        snprintf(line, sizeof(line), "%-34s threads %4d  VGPRs %3d  scratch %4zu B  LDS %6d B dynamic + %5zu B static  "
                 "blocks/CU %d (geometry needs %d)\n", what, threads, attr.numRegs, (size_t)attr.localSizeBytes,
                 lds_bytes, (size_t)attr.sharedSizeBytes, resident, blocks_per_cu);
        std::lock_guard<std::mutex> lock(g_resources_mutex);
        g_resources += line;
    }
    if (resident < blocks_per_cu) {
        // The launch is still correct (the surplus blocks queue behind the resident ones), only slower: by default this
        // is a WARNING line in fe_kernel_resources().  FEINSUM_STRICT_RESIDENCY=1 (the test suite and bench.py set it)
        // turns it into FE_EHIP, so that a compiler regression cannot pass with green tests at half the speed.
        char line[320];
        snprintf(line, sizeof(line), "WARNING %s: %d block(s) of %d threads fit a CU but the launch geometry assumes %d "
                 "(%d VGPRs, %d B of LDS per block): the compiled kernel's register or LDS use grew\n",
                 what, resident, threads, blocks_per_cu, attr.numRegs, lds_bytes);
        {
            std::lock_guard<std::mutex> lock(g_resources_mutex);
            g_resources += line;
        }
        const char* strict = getenv("FEINSUM_STRICT_RESIDENCY");
        if (strict && strict[0] == '1') return fail(FE_EHIP, "%s", line + 8);
    }
    return FE_OK;
}

// configure_kernel under the caller's once-flag: every kernel INSTANTIATION has a flag of its own, so that a
// shortfall (or any other failure) of one instantiation -- say the opt-in prepared-operator one -- cannot fail the
// launches of its siblings for the rest of the process.
template <typename Once, typename K>
int configured(Once& once, K kernel, const char* what, int lds_bytes, int threads, int blocks_per_cu) {
    return once.run([&] { return configure_kernel(kernel, what, lds_bytes, threads, blocks_per_cu); });
}

// Kernel attributes are per device: a `static std::once_flag` per kernel would configure only
// the first device a process uses.  One flag per (call site, device).
struct PerDeviceOnce {
    std::once_flag flags[64];
    int rc[64] = {};
    template <typename F>
    int run(F&& f) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
        std::call_once(flags[dev], [&] { rc[dev] = f(); });
        return rc[dev];
    }
};

}  // namespace
#include "fe_split_alloc.h"
namespace {

// ---- the argument check of the DG entry points: one description of a call, one precedence ("the front end").
//  1. structure -- E < 0, non-positive sizes, b < 1, stray flag bits, non-finite alpha / beta, a null pointer table, a leading
//     dimension below E or too large, alignment: FE_EINVAL;
//  2. scope -- no kernel for the shape, the field count or the variant: FE_EUNSUPPORTED;
//  3. E == 0: kCheckDone, the caller returns FE_OK;
//  4. null device or field pointers, E*Np too large: FE_EINVAL.
// The entry points on element slices keep the order their tests pin: scope first (CallCheck::scope_first).
// Everything here comes before any device work.
constexpr int kCheckDone = 1;
enum CheckScope { kScopeAny, kScopeTet, kScopeTetFaces };   // kernels for: any shape / tetrahedra p = 1..4 by Np / by (nf, Np, Nfp, b)
struct CallCheck {
    const char* who;
    const void* J;
    const void* op;
    const void* const* in;    // b pointers each
    const void* const* out;
    int64_t E;
    int32_t Np, b, flags, flag_mask;
    const char* flag_name = "operator";
    int in_align = 8;                       // 4: float32 fields
    int out_align = 8;                      // 4: float32 results
    const double* alpha = nullptr;          // with beta: an accumulating call
    const double* beta = nullptr;
    int64_t ld[3] = {0, 0, 0};              // ldJ, ldIn, ldOut of a call on an element slice, where ld_used
    bool ld_used[3] = {false, false, false};
    bool faces = false;                     // a face-mass call: nf, Nfp
    int32_t nf = 0, Nfp = 0;
    CheckScope scope = kScopeAny;
    const char* kernel = "kernel";          // what the scope message says is missing
    int min_b = 1;
    bool scope_first = false;               // the slice entry points: the scope comes before the structure (tests pin it)
    int variant = FE_VARIANT_AUTO, variant_hi = FE_VARIANT_AUTO;
    const void* op2 = nullptr;              // a second operator (the weighted element operator), where has_op2
    bool has_op2 = false;
};

int check_scope(const CallCheck& c) {
    const char* who = c.who;
    if (c.variant < FE_VARIANT_AUTO || c.variant > c.variant_hi) return fail(FE_EUNSUPPORTED, "%s: unknown variant %d", who, c.variant);
    if (c.scope == kScopeTet && !fe::is_tet_order(c.Np))
        return fail(FE_EUNSUPPORTED, "%s: Np = %d has no %s (tetrahedra p = 1..4: Np = 4, 10, 20, 35)", who, c.Np, c.kernel);
    // (a field count below one is malformed, not out of scope)
    if (c.scope == kScopeTetFaces && !(c.nf == fe::kFmNf && fe::is_tet_order(c.Np, c.Nfp) && !(c.b >= 1 && c.b < c.min_b)))
        return fail(FE_EUNSUPPORTED, "%s: (nf, Np, Nfp, b) = (%d, %d, %d, %d) has no %s (tetrahedra p = 1..4, b >= %d)", who, c.nf,
                    c.Np, c.Nfp, c.b, c.kernel, c.min_b);
    return FE_OK;
}

int check_call(const CallCheck& c) {
    const char* who = c.who;
    if (c.scope_first)
        if (int rc = check_scope(c)) return rc;
    if (c.E < 0) return fail(FE_EINVAL, "%s: E must be >= 0 (got %lld)", who, (long long)c.E);
    if (c.faces && (c.Np <= 0 || c.nf <= 0 || c.Nfp <= 0 || c.b <= 0))
        return fail(FE_EINVAL, "%s: Np, nf, Nfp, b must be positive (%d %d %d %d)", who, c.Np, c.nf, c.Nfp, c.b);
    if (c.Np <= 0) return fail(FE_EINVAL, "%s: Np must be positive (got %d)", who, c.Np);
    if (c.b < 1) return fail(FE_EINVAL, "%s: b=%d, need at least one field", who, c.b);
    if (c.flags & ~c.flag_mask) return fail(FE_EINVAL, "%s: bad %s flags %d", who, c.flag_name, c.flags);
    if (c.alpha && (!std::isfinite(*c.alpha) || !std::isfinite(*c.beta)))
        return fail(FE_EINVAL, "%s: alpha and beta must be finite (got %g, %g)", who, *c.alpha, *c.beta);
    if (!c.in || !c.out) return fail(FE_EINVAL, "%s: null pointer table", who);
    for (int i = 0; i < 3; ++i)
        if (c.ld_used[i] && c.ld[i] < c.E)
            return fail(FE_EINVAL, "%s: a leading dimension is smaller than E = %lld (ldJ %lld, ldIn %lld, ldOut %lld)", who,
                        (long long)c.E, (long long)c.ld[0], (long long)c.ld[1], (long long)c.ld[2]);
    for (int i = 0; i < 3; ++i)
        if (c.ld_used[i] && c.ld[i] >= (int64_t)1 << 40)
            return fail(FE_EINVAL, "%s: leading dimension too large (%lld)", who, (long long)c.ld[i]);
    if ((reinterpret_cast<uintptr_t>(c.J) | reinterpret_cast<uintptr_t>(c.op) | reinterpret_cast<uintptr_t>(c.op2)) & 7u)
        return fail(FE_EINVAL, "%s: device pointers must be 8-byte aligned (float64 arrays: J and the operator)", who);
    for (int k = 0; k < c.b; ++k) {
        if (reinterpret_cast<uintptr_t>(c.in[k]) & (uintptr_t)(c.in_align - 1))
            return fail(FE_EINVAL, c.in_align == 4 ? "%s: field %d must be 4-byte aligned (a float32 array)"
                                                   : "%s: field %d: device pointers must be 8-byte aligned (float64 arrays)", who, k);
        if (reinterpret_cast<uintptr_t>(c.out[k]) & (uintptr_t)(c.out_align - 1))
            return fail(FE_EINVAL, c.out_align == 4 ? "%s: output %d must be 4-byte aligned (a float32 array)"
                                                    : "%s: output %d: device pointers must be 8-byte aligned (float64 arrays)", who, k);
    }
    if (!c.scope_first)
        if (int rc = check_scope(c)) return rc;
    if (c.E == 0) return kCheckDone;
    if (!c.J || !c.op || (c.has_op2 && !c.op2)) return fail(FE_EINVAL, "%s: null device pointer", who);
    for (int k = 0; k < c.b; ++k)
        if (!c.in[k] || !c.out[k]) return fail(FE_EINVAL, "%s: null field pointer %d (a null device pointer)", who, k);
    if (c.E * (int64_t)c.Np >= (int64_t)1 << 39) return fail(FE_EINVAL, "%s: E*Np too large (%lld)", who, (long long)(c.E * c.Np));
    return FE_OK;
}

template <typename T>
const void* const* ptr_table(T* const* p) { return reinterpret_cast<const void* const*>(p); }
void use_ld(CallCheck& c, int i, int64_t ld) { c.ld[i] = ld; c.ld_used[i] = true; }
#define FE_CHECK_CALL(c) \
    if (int rc_ = check_call(c)) return rc_ == kCheckDone ? FE_OK : rc_

// the older entry points check field by field, and an empty call goes on to their own checks of flags and variant
int check_common(const char* who, const void* J, const void* D, const void* u, const void* out, int64_t E, int32_t Np) {
    const CallCheck c = {who, J, D, &u, &out, E, Np, 1, 0, 0};
    const int rc = check_call(c);
    return rc == kCheckDone ? FE_OK : rc;
}

unsigned generic_grid(int64_t E, int Np) { return (unsigned)((E * Np + 255) / 256); }

// ---- dynamic walk (fe_common.h): the ticket counters of a launch.
// Who may share counters: nobody who can run at the same time.  A launch's counters are zero before and after it (the
// kernels clean up behind themselves), so launches that the device SERIALISES may use the same ones; launches that can
// overlap must not (two launches drawing from one counter take each other's tiles -- silently).  Ownership therefore
// follows what orders launches:
//  * an eager launch uses the counter group of ITS STREAM (a per-device map stream -> group; the per-thread default
//    stream is a different stream in every thread and is keyed by the thread).  Launches on one stream run one after the
//    other; two streams -- driven from one host thread or from several -- never share a group;
//  * a launch recorded during stream capture gets a group of ITS OWN, for good: the graph node bakes the pointer in and
//    may be replayed on any stream beside any eager launch (launches of one executable graph are ordered by HIP);
//  * a group is four consecutive counter sets (a fused launch uses one set per body);
//  * groups come from chunks of kTailChunkGroups, allocated and zeroed outside stream capture only (a capture that finds
//    no spare group walks statically, and so does everything once kTailMaxGroups exist: the static walk needs no state);
//  * fe_stream_retired() returns a destroyed stream's group; fe_tail_check() verifies the zero-between-launches invariant
//    on an idle device (and repairs it), FEINSUM_TAIL_CHECK=1 does so before every dynamic launch (debugging aid: it
//    synchronises the stream).
// Round 5 closes three edges of that scheme:
//  * ONE EXECUTABLE PER CAPTURE.  The group pointer is baked into the graph NODE: every executable instantiated from one
//    captured graph uses the same counters, and HIP orders only the launches of one executable.  Two executables of one
//    capture must not run at the same time (include/feinsum_hip.h says so; BoundOperator.capture() instantiates one).
//  * captured groups come back: the groups a capture took are recorded under the capture's id (fe_capture_id), and
//    fe_graph_retired(id) returns them once the caller has destroyed the graph -- an application that re-captures every
//    step no longer runs out of groups after kTailMaxGroups captures and falls back to the static walk for good;
//    fe_tail_stats reports `exhausted` and `static_fallbacks` so that the fallback is visible;
//  * a failed chunk allocation is retried (not latched), and after any FE_EHIP return of the process the first dynamic
//    launch of every stream verifies (and repairs) its group once -- the checked mode is no longer opt-in where it matters.
constexpr int kTailSetsPerGroup = 4;
constexpr int kTailChunkGroups = 16;                     // 8.9 MB per chunk
constexpr int kTailMaxGroups = 256;                      // per device
constexpr size_t kTailGroupWords = (size_t)kTailSetsPerGroup * fe::kTailWords;
struct TailPool {
    std::mutex lock;
    std::unordered_map<uintptr_t, unsigned*> by_stream;   // eager launches
    std::unordered_map<uintptr_t, unsigned> verified_at;  // per stream: the FE_EHIP epoch its group was last verified at
    std::unordered_map<unsigned long long, std::vector<unsigned*>> by_capture;   // capture id -> the groups its nodes own
    std::vector<unsigned*> spare;                          // zeroed groups nobody owns
    std::vector<unsigned*> chunks;                         // every allocation (fe_tail_check walks them)
    int groups = 0, captured = 0;
    long long exhausted = 0;          // launches that found no group (all kTailMaxGroups owned, or none spare during capture)
    long long static_fallbacks = 0;   // launches that wanted tickets and walked statically (exhausted, failed allocation, HIP errors)
    long long grow_failures = 0;      // chunk allocations that failed (retried by later launches)
    long long verified_after_error = 0, repaired_after_error = 0;
    int failed_recently = 0;          // launches to wait before the next allocation attempt
    hipStream_t zero_stream = nullptr;
    // a fresh chunk: zeroed through a stream of our own and waited for, so that whoever takes a group later -- on any
    // stream -- finds zeros without being ordered behind anything
    bool grow() {
        if (groups + kTailChunkGroups > kTailMaxGroups) return false;
        // a failed allocation (say during another thread's global-mode capture) is not final: the launches walk statically
        // meanwhile and the 64th of them tries again
        if (failed_recently > 0) { --failed_recently; return false; }
        unsigned* p = nullptr;
        const size_t bytes = (size_t)kTailChunkGroups * kTailGroupWords * sizeof(unsigned);
        bool ok = zero_stream || hipStreamCreateWithFlags(&zero_stream, hipStreamNonBlocking) == hipSuccess;
        ok = ok && hipMalloc(&p, bytes) == hipSuccess;
        ok = ok && hipMemsetAsync(p, 0, bytes, zero_stream) == hipSuccess && hipStreamSynchronize(zero_stream) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            if (p) (void)hipFree(p);
            ++grow_failures;
            failed_recently = 64;
            return false;
        }
        chunks.push_back(p);
        for (int g = kTailChunkGroups - 1; g >= 0; --g) spare.push_back(p + (size_t)g * kTailGroupWords);
        groups += kTailChunkGroups;
        return true;
    }
};
TailPool g_tail[64];
std::atomic<int> g_tail_check{[] { const char* e = getenv("FEINSUM_TAIL_CHECK"); return e && e[0] == '1' ? 1 : 0; }()};

uintptr_t tail_stream_key(hipStream_t s) {
    if (s == hipStreamPerThread) {   // one handle value, a different stream in every thread
        static thread_local char marker;
        return reinterpret_cast<uintptr_t>(&marker) | 1u;
    }
    return reinterpret_cast<uintptr_t>(s);
}

// counts (and clears) the non-zero words of a group; the caller has made sure nothing is running on it
int tail_group_dirty(unsigned* group, bool repair, long long* dirty) {
    static thread_local std::vector<unsigned> host;
    host.resize(kTailGroupWords);
    FE_HIP_CHECK(hipMemcpy(host.data(), group, kTailGroupWords * sizeof(unsigned), hipMemcpyDeviceToHost));
    long long n = 0;
    for (unsigned w : host) n += w != 0;
    if (n && repair) FE_HIP_CHECK(hipMemset(group, 0, kTailGroupWords * sizeof(unsigned)));
    *dirty += n;
    return FE_OK;
}

// The counters for a launch on stream `s` that needs `sets` consecutive sets; null = walk statically.
unsigned* tail_slot(hipStream_t s, int sets = 1) {
    int dev = 0;
    if (sets < 1 || sets > kTailSetsPerGroup) return nullptr;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    TailPool& pool = g_tail[dev];
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    unsigned long long capture_id = 0;
    if (hipStreamGetCaptureInfo(s, &st, &capture_id) != hipSuccess) {
        (void)hipGetLastError();
        std::lock_guard<std::mutex> guard(pool.lock);
        ++pool.static_fallbacks;
        return nullptr;
    }
    std::lock_guard<std::mutex> guard(pool.lock);
    if (st != hipStreamCaptureStatusNone) {   // a graph node: a group of its own until fe_graph_retired(capture id)
        if (pool.spare.empty()) {              // (no allocation during capture)
            ++pool.exhausted;
            ++pool.static_fallbacks;
            return nullptr;
        }
        unsigned* g = pool.spare.back();
        pool.spare.pop_back();
        ++pool.captured;
        pool.by_capture[capture_id].push_back(g);
        return g;
    }
    const uintptr_t key = tail_stream_key(s);
    auto it = pool.by_stream.find(key);
    if (it == pool.by_stream.end()) {
        // keep a chunk's worth of spares behind the eager streams, so that a later capture finds some
        if (pool.spare.size() <= 1 && !pool.grow() && pool.spare.empty()) {
            if (pool.groups + kTailChunkGroups > kTailMaxGroups) ++pool.exhausted;
            ++pool.static_fallbacks;
            return nullptr;
        }
        unsigned* g = pool.spare.back();
        pool.spare.pop_back();
        it = pool.by_stream.emplace(key, g).first;
        pool.verified_at[key] = g_hip_error_epoch.load(std::memory_order_relaxed);   // fresh from the spares: zero
    }
    // after any FE_EHIP return of the process a launch may have stopped half way: the first dynamic launch of every stream
    // behind it verifies its group once (it waits for the stream: rare, and only after an error); FEINSUM_TAIL_CHECK=1 does
    // so before EVERY dynamic launch (debugging aid)
    const unsigned epoch = g_hip_error_epoch.load(std::memory_order_relaxed);
    unsigned& seen = pool.verified_at[key];
    const bool after_error = seen != epoch;
    if (after_error || g_tail_check.load(std::memory_order_relaxed)) {
        long long dirty = 0;
        const bool ok = hipStreamSynchronize(s) == hipSuccess && tail_group_dirty(it->second, true, &dirty) == FE_OK;
        if (!ok) (void)hipGetLastError();
        if (after_error) {
            ++pool.verified_after_error;
            if (dirty) ++pool.repaired_after_error;
            if (ok) seen = epoch;
        }
        if (!ok || dirty)
            fprintf(stderr, "feinsum_hip: ticket counters of stream %p held %lld non-zero words before a launch (%s)\n",
                    (void*)s, dirty, ok ? "repaired" : "could not be verified: static walk");
        if (!ok) {
            ++pool.static_fallbacks;
            return nullptr;
        }
    }
    return it->second;
}
// Number of statically walked tiles of a launch of `blocks` blocks of `waves / blocks` waves: two rounds, the rest by
// tickets (FEINSUM_TAIL_ROUNDS / fe_set_tail_rounds: at most so many full rounds by tickets; negative: none); launches of
// fewer than four and a half rounds walk statically (E = 1e5 on 2048 waves: three rounds, measured slower with tickets), and so do
// grids of fewer than 8 blocks per pool: a block's pool is (bid / 8) % kTailPools and nobody steals, so that a pool
// without blocks would keep its tiles (a 32-CU partition launches 64 blocks).
std::atomic<int> g_tail_rounds{[] { const char* e = getenv("FEINSUM_TAIL_ROUNDS"); return e ? atoi(e) : (1 << 20); }()};
// (experiments: FEINSUM_TAIL_MIN_ROUNDS lowers the four-round rule below, to re-measure tickets in shorter launches)
std::atomic<int> g_tail_min_rounds_v{[] { const char* e = getenv("FEINSUM_TAIL_MIN_ROUNDS"); return e ? atoi(e) : 4; }()};
#define g_tail_min_rounds g_tail_min_rounds_v.load(std::memory_order_relaxed)
// `fused`: a body of a fused launch (div + grad, div + grad + lift) walks dynamically from THREE rounds on -- the bodies of a block
// follow each other, so a block that is late in one body starts the next late, and tickets absorb that: div + grad at E = 1e5
// 46.1 -> 43.4 us, the pipeline 103.9 -> 97.5, -1 ... -6 % at every size between three and four and a half rounds, level at exact
// multiples (profiles/r05/fused_tickets3_ab.txt); single launches lose up to 8 % there (single_tickets3_ab.txt) and keep four.
// `units`: a face-mass launch of four fields (p = 4) walks four units per tile, so a ticket's round trip hides behind more work: it
// gains from tickets from three rounds on as the fused launches do -- E = 1e5 52.3 -> 51.0 us, 1.2e5 -3.6 %, 1.4e5 -2.3 %, level
// at 1.1e5 -- except where the tiles fill whole rounds, which are balanced as they are (98 304: +3.6 % with tickets;
// profiles/r05/facemass_tickets_from_three_rounds_ab.txt).
int64_t tail_static_tiles(int64_t nTiles, int64_t blocks, int wavesPerBlock, bool fused = false, bool units = false) {
    const int dyn_rounds = g_tail_rounds.load(std::memory_order_relaxed);
    const int64_t waves = blocks * wavesPerBlock;
    const int64_t rounds = waves > 0 ? nTiles / waves : 0;
    const int min_rounds = ((fused || units) && g_tail_min_rounds == 4) ? 3 : g_tail_min_rounds;
    if (blocks < 8 * fe::kTailPools) return nTiles;
    if (dyn_rounds < 0 || rounds < min_rounds || nTiles >= ((int64_t)1 << 29)) return nTiles;   // (32-bit ticket arithmetic: fe_common.h)
    if (units && !fused && rounds <= 4 && nTiles == rounds * waves) return nTiles;
    // four rounds and a bit: tickets pay once the partial fifth round is at least half a round -- a static walk leaves those waves
    // a tile behind the rest (div E = 163 000: 41.2 -> 37.7 us; grad 150 000: 34.4 -> 33.5), while four EXACT rounds are perfectly
    // balanced as they are (grad 131 072: 28.6 static, 30.7 with tickets; profiles/r04/dynamic_walk_from_four_and_a_half_rounds.txt)
    if (rounds == 4 && min_rounds == 4 && (nTiles - 4 * waves) * 2 < waves) return nTiles;
    int64_t ks = rounds - dyn_rounds;
    if (ks < 2) ks = 2;
    return ks * waves;
}

// kOpLoadsTemporal (fe_common.h) for a launch that reads `input_bytes`: plain instead of non-temporal loads of the streamed
// operand while the launch's inputs fit the Infinity Cache ($FEINSUM_TEMPORAL_LOADS_MIB / fe_set_temporal_loads_mib; 0 = never).
// `min_bytes`: div and face-mass launches of fewer than about three rounds measured 3 - 8 % SLOWER with plain loads (div
// E = 4e4 ... 8e4, face-mass x 4 E = 2e4 ... 3e4; grad and the fused launches gain or stay level at every small size:
// profiles/r04/temporal_loads_ab.txt), so those families switch only above a measured floor.
std::atomic<long long> g_temporal_input_bytes{[] {
    const char* e = getenv("FEINSUM_TEMPORAL_LOADS_MIB");
    return e ? (long long)atoll(e) << 20 : fe::kTemporalInputBytes;
}()};
// `cap_mib`: up to which size of its inputs a family's launches gain from plain loads -- more than the cache holds for the
// families whose footprint is mostly inputs: what the cache holds of them is found again.  Measured (profiles/r05/
// temporal_loads_fused_ab.txt, back-to-back launches on the same arrays): grad gains up to 235 - 245 MiB and loses 1.5 ... 12 % from
// 245 - 270 on (kTemporalInputBytes = 248 MiB); div gains up to 270 MiB (-4 %), is level at 287 and loses 6 % at 304; div + grad gains
// up to 301 MiB (-2 %; 253 MiB: -8 %) and loses at 326; launches with face-mass in them -- face-mass alone, the wave operator --
// gain up to 316 - 325 MiB (the pipeline at E = 1e5, 307 MiB: 99.6 -> 94.8 us; face-mass x 4 at 1.5e5, 279 MiB: 80.7 -> 72.3) and lose
// 2 ... 4 % at 335 - 370.  The caller's setting (fe_set_temporal_loads_mib; 0 = never) scales every family's cap alike.
constexpr long long kTemporalCapGradMib = 248, kTemporalCapDivMib = 280, kTemporalCapGradDivMib = 310, kTemporalCapFaceMassMib = 320;
int temporal_flag(int64_t input_bytes, int64_t min_bytes = 0, long long cap_mib = kTemporalCapGradMib) {
    long long cap = g_temporal_input_bytes.load(std::memory_order_relaxed);
    if (cap >= (1ll << 40)) return fe::kOpLoadsTemporal;        // "always" (A/B runs)
    cap = cap / kTemporalCapGradMib * cap_mib;
    return input_bytes <= cap && input_bytes >= min_bytes ? fe::kOpLoadsTemporal : 0;
}
constexpr int64_t kTemporalFloorDiv = 80ll << 20, kTemporalFloorFaceMass = 64ll << 20;

// kOpStoresWriteThrough (fe_common.h) for a launch that writes `output_bytes` ($FEINSUM_WRITE_THROUGH_MIB /
// fe_set_write_through_mib; 0 = never)
std::atomic<long long> g_write_through_output_bytes{[] {
    const char* e = getenv("FEINSUM_WRITE_THROUGH_MIB");
    return e ? (long long)atoll(e) << 20 : fe::kWriteThroughOutputBytes;
}()};
int write_through_flag(int64_t output_bytes) {
    return output_bytes <= g_write_through_output_bytes.load(std::memory_order_relaxed) ? fe::kOpStoresWriteThrough : 0;
}

// short div launches (static walk) on the kernel whose B build is interleaved into the matrix phase (fe_div.h, kIlv): launches of
// at most so many tiles ($FEINSUM_DIV_INTERLEAVE_TILES / fe_set_div_interleave; 0 = never)
// Measured (profiles/r05/div_interleave_ab.txt, div_interleave_small.txt; same arrays, in-process): -3 ... -6 % at E = 8e4 ... 3e5 under
// either walk, -2 % at 4e5, level from 6e5 on (the launch is memory bound there) -- hence the default of 37 500 tiles (E = 6e5).
constexpr long long kDivInterleaveTiles = 37500;
std::atomic<long long> g_div_interleave_tiles{[] { const char* e = getenv("FEINSUM_DIV_INTERLEAVE_TILES"); return e ? atoll(e) : kDivInterleaveTiles; }()};

// ... and the tiles behind the last full round of such a launch as quarter tiles (fe_div.h, kOpQuarterTail): $FEINSUM_DIV_QUARTER_TAIL /
// fe_set_div_quarter_tail
std::atomic<int> g_div_quarter_tail{[] { const char* e = getenv("FEINSUM_DIV_QUARTER_TAIL"); return e ? atoi(e) : 1; }()};

// ... and of short grad launches (fe_grad.h; one field, static walk, one sub-tile per wave tile): $FEINSUM_GRAD_QUARTER_TAIL /
// fe_set_grad_quarter_tail.  The rule is the kernel's own (at least one full round, the ragged one at most an eighth full).
constexpr int kGradQuarterDen = 8;
std::atomic<int> g_grad_quarter_tail{[] { const char* e = getenv("FEINSUM_GRAD_QUARTER_TAIL"); return e ? atoi(e) : 1; }()};
int grad_quarter_flag(int m, int nb, int64_t nTiles, int64_t waves) {
    const int64_t ragged = nTiles % waves;
    const int setting = g_grad_quarter_tail.load(std::memory_order_relaxed);   // 0 off, 1 the default rule, n >= 4: ragged <= waves / n
    const int64_t den = setting >= 4 ? setting : kGradQuarterDen;
    return (m == 1 && nb == 1 && setting != 0 && nTiles > waves && ragged > 0 && den * ragged <= waves) ? fe::kOpQuarterTail : 0;
}

// ... and whether the odd CUs of every XCD start such a launch half a tile period late (fe_common.h, kOpStaggeredStart):
// $FEINSUM_GRAD_STAGGERED_START / fe_set_grad_staggered_start.  The rule: tetrahedra p = 4, one field, a full grid, at least 2.5
// rounds of tiles (the static walk ends at 4.5 rounds by itself).
std::atomic<int> g_grad_staggered_start{[] { const char* e = getenv("FEINSUM_GRAD_STAGGERED_START"); return e ? atoi(e) : 1; }()};
int grad_stagger_flag(int np, int m, int nb, int64_t nTiles, int64_t waves) {
    return (np == 35 && m == 1 && nb == 1 && g_grad_staggered_start.load(std::memory_order_relaxed) && 2 * nTiles >= 5 * waves) ? fe::kOpStaggeredStart : 0;
}

// the same flag for the eight-wave p = 5 kernels (compute bound at every size): $FEINSUM_PHASE_PRIORITY_P5 / fe_set_phase_priority_p5
std::atomic<int> g_phase_priority_p5{[] { const char* e = getenv("FEINSUM_PHASE_PRIORITY_P5"); return e ? atoi(e) : 0; }()};
int phase_priority_flag_p5() { return g_phase_priority_p5.load(std::memory_order_relaxed) ? fe::kOpPhasePriority : 0; }

// What the launcher decided for the MFMA launch enqueued last by this thread (fe_last_launch_info): bench.py and the tools report
// these instead of re-deriving the rules (round 4's report recomputed them in Python and could disagree with the kernel).
struct LastLaunch {
    int valid = 0, dynamic_walk = 0, temporal_loads = 0, write_through = 0, blocks = 0, waves_per_block = 0, kind = 0, bodies = 0;
    long long tiles = 0, static_tiles = 0;
};
thread_local LastLaunch g_last_launch;
// (at the entry of every family's entry point: a call that runs only tiled or generic kernels reports no launch)
void forget_last_launch() { g_last_launch.valid = 0; }
void note_launch(bool dynamic, int flags, unsigned blocks, int waves_per_block, int64_t tiles, int64_t static_tiles, int kind = 0, int bodies = 1) {
    LastLaunch& L = g_last_launch;
    L.valid = 1;
    L.dynamic_walk = dynamic ? 1 : 0;
    L.temporal_loads = (flags & fe::kOpLoadsTemporal) ? 1 : 0;
    L.write_through = (flags & fe::kOpStoresWriteThrough) ? 1 : 0;
    L.blocks = (int)blocks;
    L.waves_per_block = waves_per_block;
    L.kind = kind;
    L.bodies = bodies;
    L.tiles = tiles;
    L.static_tiles = dynamic ? static_tiles : tiles;
}

// Persistent-style grid: a block per `wavesPerBlock` tiles, at most `per_cu` blocks per CU.
// (a per-wave-equal grid -- every wave the same number of tiles, on fewer waves -- was measured in round 3 and is slower at
// every size: profiles/r03/balanced_grid_ab.txt)
unsigned grid_for(int64_t nTiles, int wavesPerBlock, int per_cu) {
    const int64_t blocks = (nTiles + wavesPerBlock - 1) / wavesPerBlock;
    const int64_t cap = per_cu * (int64_t)device_cu_count();
    return (unsigned)(blocks < cap ? blocks : cap);
}
// ... of 8 waves per CU (2 blocks of 4 waves: the VGPR / LDS residency of the per-wave-tile kernels)
unsigned persistent_grid(int64_t nTiles, int wavesPerBlock) { return grid_for(nTiles, wavesPerBlock, 8 / wavesPerBlock); }

// ---- one persistent MFMA launch: every DG family launcher goes through mfma_launch below, which owns the four rules the
// launchers share -- which once-flag configures a kernel, how large the grid is, which walk the launch takes, what is recorded.

// configure_kernel once per (kernel INSTANTIATION, device): the flag is keyed on the kernel itself.  Many instantiations share
// one signature (grad3d_mfma_kernel<35, 1, 0> and <20, 2, 0>); a flag keyed on the pointer's type would configure only the
// first of them and silently skip the LDS attribute of the rest.  A failure of one instantiation (say the opt-in
// prepared-operator one) cannot fail the launches of its siblings for the rest of the process.
template <auto K>
int configured(const char* what, int lds_bytes, int threads, int blocks_per_cu) {
    static PerDeviceOnce once;
    return once.run([&] { return configure_kernel(K, what, lds_bytes, threads, blocks_per_cu); });
}

// A kernel's launch geometry: blocks of `waves` waves (`threads` threads, `lds` bytes of dynamic LDS), `resident` of them per
// CU (configure_kernel checks that), and the launcher's grid rule: at most `per_cu` blocks per CU.
struct Geometry {
    int waves, threads, lds, resident, per_cu;
};

// Which tiles may come by tickets (fe_common.h, dynamic walk): bit b of `tickets` for body b -- one body, or the div, grad and
// lift bodies of a fused launch, each walked on its own over one counter set of a group (tail_slot(s, bodies)).
struct Walk {
    int64_t tiles[3];
    int bodies;
    unsigned tickets;
    bool units;   // tail_static_tiles' `units` (face-mass x 4); its `fused` is bodies > 1
};
Walk walk_static(int64_t tiles) { return {{tiles, 0, 0}, 1, 0u, false}; }
Walk walk_tickets(int64_t tiles, bool tickets = true, bool units = false) { return {{tiles, 0, 0}, 1, tickets ? 1u : 0u, units}; }

// What mfma_launch decided: the grid, the tiles each body walks statically, the counters of a dynamic walk (or null).
struct Launch {
    unsigned grid;
    int waves_per_block;
    int64_t t_static[3];
    unsigned* tail;
    int64_t waves() const { return (int64_t)grid * waves_per_block; }
};

// The kernel arguments of one launch, with the flags and `kind` bits (fe_last_launch_info) recorded for it.
template <typename... A>
struct Call {
    int flags, kind;
    std::tuple<A...> args;
};
template <typename... A>
Call<A...> call(int flags, int kind, A... args) { return {flags, kind, std::tuple<A...>(args...)}; }

// Configure K (and KT when it runs), size the grid, walk statically or by tickets, enqueue, record.  `static_call(L)` gives K's
// arguments; when tickets were granted and KT is a kernel, `tail_call(L)` gives KT's (the counters are L.tail, behind
// L.t_static[0] tiles).  A null KT walks statically -- except a fused launch, whose kernel takes the counters itself: it passes
// itself as KT and the same arguments for both.
template <auto K, auto KT = nullptr, typename SC, typename TC = std::nullptr_t>
int mfma_launch(hipStream_t s, const Walk& w, const Geometry& g, const char* what, SC static_call, const char* tail_what = nullptr,
                TC tail_call = nullptr) {
    if (int rc = configured<K>(what, g.lds, g.threads, g.resident)) return rc;
    int64_t most = 0, tiles = 0, t_static = 0;
    for (int b = 0; b < w.bodies; ++b) {
        most = w.tiles[b] > most ? w.tiles[b] : most;
        tiles += w.tiles[b];
    }
    Launch L = {grid_for(most, g.waves, g.per_cu), g.waves, {w.tiles[0], w.tiles[1], w.tiles[2]}, nullptr};
    bool dynamic = false;
    if constexpr (KT != nullptr) {
        for (int b = 0; b < w.bodies; ++b)
            if (w.tickets & (1u << b)) {
                L.t_static[b] = tail_static_tiles(w.tiles[b], L.grid, g.waves, w.bodies > 1, w.units);
                dynamic = dynamic || L.t_static[b] < w.tiles[b];
            }
        if (dynamic) L.tail = tail_slot(s, w.bodies);
    }
    for (int b = 0; b < w.bodies; ++b) t_static += L.t_static[b];
    auto enqueue = [&](auto kernel, const auto& c) {
        std::apply([&](auto... a) { hipLaunchKernelGGL(kernel, dim3(L.grid), dim3(g.threads), g.lds, s, a...); }, c.args);
        note_launch(L.tail != nullptr, c.flags, L.grid, g.waves, tiles, t_static, c.kind, w.bodies);
        return FE_OK;
    };
    if constexpr (KT != nullptr) {
        if (L.tail) {
            if (int rc = configured<KT>(tail_what, g.lds, g.threads, g.resident)) return rc;
            return enqueue(KT, tail_call(L));
        }
    }
    return enqueue(K, static_call(L));
}

// The p = 5 kernels (Np = 56): eight waves per block share the A fragments in LDS, one block per CU
template <typename G>
constexpr Geometry w8_geometry() { return {G::WAVES, G::THREADS, G::LDS_BYTES, G::BLOCKS_PER_CU, 1}; }

// grad of tetrahedra p = 5: grad by components
int launch_grad_p5(const double* J, const double* D, const fe::FieldPtrs& P, int nb, int64_t E, int opT,
                   hipStream_t s, bool* launched, int dbg = 0) {
    using G = fe::DivGeom<56, 1, 4, 3, true, true>;
    const int64_t nTiles = E / G::TEL;
    *launched = nTiles > 0;   // the launch covers the elements behind the last tile too
    if (nTiles == 0) return FE_OK;
    opT |= phase_priority_flag_p5();
    auto args = [&](const Launch&) { return call(opT, 0, J, D, nullptr, P, nb, E, nTiles, opT, 0); };
#ifdef FE_EXPERIMENTS
#define FE_P5_CASE(DBG) \
    case DBG: return mfma_launch<fe::div3d_mfma_kernel<56, 1, DBG, 4, 3, true, true>>(s, walk_static(nTiles), w8_geometry<G>(), "experiment", args);
    switch (dbg) {
        FE_P5_CASE(1) FE_P5_CASE(2) FE_P5_CASE(3) FE_P5_CASE(4) FE_P5_CASE(5) FE_P5_CASE(6) FE_P5_CASE(8) FE_P5_CASE(9) FE_P5_CASE(10) FE_P5_CASE(11) FE_P5_CASE(32) FE_P5_CASE(16) FE_P5_CASE(64) FE_P5_CASE(80)
        default: break;
    }
#undef FE_P5_CASE
#else
    (void)dbg;
#endif
    // one field: behind two static rounds the tiles come by tickets (fe_common.h, dynamic walk)
    return mfma_launch<fe::div3d_mfma_kernel<56, 1, 0, 4, 3, true, true>, fe::grad_w8_tail_kernel<56>>(
        s, walk_tickets(nTiles, nb == 1), w8_geometry<G>(), "grad p5 (components, A in LDS)", args,
        "grad p5 (components, A in LDS), dynamic walk",
        [&](const Launch& L) { return call(opT, 0, J, D, P, nb, E, nTiles, opT, L.tail, L.t_static[0]); });
}

// grad-type planes of tetrahedra p = 5 (MODE 5 of the div template): D u once per field
int launch_gradplanes_p5(const fe::GradFields& Q, const double* D, int nb, int64_t E, int opT, hipStream_t s,
                         bool* launched) {
    using G = fe::DivGeom<56, 1, 5, 3, true, true>;
    const int64_t nTiles = E / G::TEL;
    *launched = nTiles > 0;   // the launch covers the elements behind the last tile too
    if (nTiles == 0) return FE_OK;
    fe::FieldPtrs P = {};
    for (int k = 0; k < nb; ++k) P.v[k] = Q.u[k];
    return mfma_launch<fe::gradplanes_bycomp_kernel<56>>(s, walk_static(nTiles), w8_geometry<G>(), "grad planes p5 (components, A in LDS)",
                                                         [&](const Launch&) { return call(opT, 0, Q, D, P, nb, E, nTiles, opT); });
}

// div of tetrahedra p = 5: the A fragments in LDS and the u planes streamed, one plane buffer per wave (round 4; round 2's four
// waves with two buffers each measured slower at E = 1e6 -- profiles/r04/p5_div_eight_waves.txt -- and were removed)
int launch_div_p5(const double* J, const double* D, const fe::FieldPtrs& P, int nb, int64_t E, int opT,
                  hipStream_t s, bool* launched) {
    using G = fe::DivGeom<56, 1, 0, 3, true, true>;
    const int64_t nTiles = E / G::TEL;
    *launched = nTiles > 0;   // the launch covers the elements behind the last tile too
    if (nTiles == 0) return FE_OK;
    opT |= phase_priority_flag_p5();
    // one field: behind two static rounds the tiles come by tickets (fe_common.h, dynamic walk)
    return mfma_launch<fe::div3d_mfma_kernel<56, 1, 0, 0, 3, true, true>, fe::div_w8_tail_kernel<56>>(
        s, walk_tickets(nTiles, nb == 1), w8_geometry<G>(), "div p5 (A in LDS, planes streamed, eight waves)",
        [&](const Launch&) { return call(opT, 0, J, D, nullptr, P, nb, E, nTiles, opT, 0); },
        "div p5 (A in LDS, planes streamed, eight waves), dynamic walk",
        [&](const Launch& L) { return call(opT, 0, J, D, P, nb, E, nTiles, opT, L.tail, L.t_static[0]); });
}

// ---- the LDS-tiled VALU kernel (fe_tiled.h): any shape whose operator fits in LDS
constexpr int64_t kTiledMaxLds = fe::kTiledLdsBudget;

bool tiled_fits(fe::TiledArgs a) { return a.Np >= 1 && a.Np <= fe::kTiledThreads && fe::tiled_plan(a) <= kTiledMaxLds; }

template <typename T>
int launch_tiled_t(fe::TiledArgs a, hipStream_t s) {
    const int64_t lds = fe::tiled_plan(a, (int)sizeof(T));
    if (a.Np > fe::kTiledThreads || lds > kTiledMaxLds)
        return fail(FE_EUNSUPPORTED, "tiled kernel: operator and tile need %lld bytes of LDS (limit %lld)",
                    (long long)lds, (long long)kTiledMaxLds);
    static PerDeviceOnce once;
    const int attr_rc = once.run([] {
        const int rc = configure_kernel(fe::tiled_apply_kernel<8, T>, sizeof(T) == 8 ? "tiled<8>" : "tiled<8> float32", (int)kTiledMaxLds,
                                        fe::kTiledThreads, 1);
        return rc != FE_OK ? rc : configure_kernel(fe::tiled_apply_kernel<4, T>, sizeof(T) == 8 ? "tiled<4>" : "tiled<4> float32",
                                                   (int)kTiledMaxLds, fe::kTiledThreads, 1);
    });
    if (attr_rc != FE_OK) return attr_rc;
    const int64_t nTiles = (a.E + a.TE - 1) / a.TE;
    int64_t per_cu = kTiledMaxLds / lds;   // resident blocks per CU: LDS, and 2048 threads
    if (per_cu > 2048 / fe::kTiledThreads) per_cu = 2048 / fe::kTiledThreads;
    const int64_t cap = per_cu * device_cu_count();
    const dim3 grid((unsigned)(nTiles < cap ? nTiles : cap)), block(fe::kTiledThreads);
    if (a.EB == 8) hipLaunchKernelGGL((fe::tiled_apply_kernel<8, T>), grid, block, (size_t)lds, s, a);
    else hipLaunchKernelGGL((fe::tiled_apply_kernel<4, T>), grid, block, (size_t)lds, s, a);
    FE_HIP_CHECK(hipGetLastError());
    return FE_OK;
}
int launch_tiled(fe::TiledArgs a, hipStream_t s) { return launch_tiled_t<double>(a, s); }

// Which kernel class serves a call.  AUTO: MFMA where compiled, else the tiled kernel where the
// operator fits in LDS, else the plain generic kernels.
enum KernelPath { kPathGeneric, kPathMfma, kPathTiled };
int choose_path(int variant, bool mfma_ok, bool tiled_ok, const char* what, int Np, KernelPath* path) {
    if (variant == FE_VARIANT_GENERIC) { *path = kPathGeneric; return FE_OK; }
    if (variant == FE_VARIANT_TILED) {
        if (!tiled_ok)
            return fail(FE_EUNSUPPORTED, "%s: the tiled kernel does not serve this call (operator too large for LDS, or "
                        "separate output planes; Np=%d)", what, Np);
        *path = kPathTiled;
        return FE_OK;
    }
    if (variant == FE_VARIANT_MFMA && !mfma_ok)
        return fail(FE_EUNSUPPORTED, "%s: MFMA variant is not compiled for this shape (Np=%d)", what, Np);
    *path = mfma_ok ? kPathMfma : tiled_ok ? kPathTiled : kPathGeneric;
    return FE_OK;
}

fe::TiledArgs tiled_args(int family, const double* J, const double* A, const fe::FieldPtrs& P, int nb, int64_t E,
                         int ndim, int Np, int nf, int Nfp, int opT, int jlayout, int rlayout) {
    fe::TiledArgs a = {};
    a.J = J; a.A = A; a.P = P; a.E = E; a.family = family;
    a.ndim = ndim; a.Np = Np; a.nf = nf; a.Nfp = Nfp; a.nb = nb;
    a.opT = opT; a.jlayout = jlayout; a.rlayout = rlayout;
    return a;
}

template <int NP, int M>
int launch_grad(const fe::GradFields& P, bool plain, const double* D, const void* prep, int nb, int nx, int64_t E,
                int dbg, int opT, hipStream_t s, int64_t* e_done) {
    using G = fe::GradGeom<NP, M>;
    const int64_t nTiles = E / G::TEL;   // full wave tiles; the remainder goes to the generic kernel
    *e_done = nTiles > 0 ? E : 0;   // the launch covers the elements behind the last tile too (remainder_items)
    if (nTiles == 0) return FE_OK;
    opT |= temporal_flag((9 + (int64_t)nb * NP) * E * 8);
    const Geometry geo = {G::WAVES, 256, G::LDS_BYTES, 2, 8 / G::WAVES};
    const void* gsec = prep ? static_cast<const char*>(prep) + fe::kPrepGradOff : nullptr;
    char what[64], tail_what[64];
    auto args = [&](const Launch&) { return call(opT, 0, P, D, nullptr, nb, nx, E, nTiles, opT); };
    auto tail_args = [&](const Launch& L) { return call(opT, 0, P, D, nb, E, nTiles, opT, L.tail, L.t_static[0]); };
    if (!plain) {   // general planes: per-plane geometry-factor and output pointers
        snprintf(what, sizeof(what), "grad planes Np=%d M=%d", NP, M);
        return mfma_launch<fe::grad3d_mfma_kernel<NP, M, 0, false>>(s, walk_static(nTiles), geo, what, args);
    }
#ifdef FE_EXPERIMENTS
    // (the per-tile stamps of 32 and 96 live behind the kernel's own LDS)
    const Geometry dbg_geo = {G::WAVES, 256, G::LDS_BYTES, 1, 8 / G::WAVES},
                   stamps_geo = {G::WAVES, 256, G::LDS_BYTES + fe::kDbgTileLdsBytes, 1, 8 / G::WAVES};
#define FE_GRAD_CASE(DBG, GEO) \
    case DBG: return mfma_launch<fe::grad3d_mfma_kernel<NP, M, DBG>>(s, walk_static(nTiles), GEO, "experiment", args);
    switch (NP == 35 ? dbg : 0) {
        FE_GRAD_CASE(1, dbg_geo)
        FE_GRAD_CASE(2, dbg_geo)
        FE_GRAD_CASE(3, dbg_geo)     // data movement in: loads only
        FE_GRAD_CASE(4, dbg_geo)     // temporal stores
        FE_GRAD_CASE(8, dbg_geo)     // no loads
        FE_GRAD_CASE(9, dbg_geo)     // stores + stage 2
        FE_GRAD_CASE(10, dbg_geo)    // arithmetic and LDS only
        FE_GRAD_CASE(11, dbg_geo)    // stage 2 and LDS only
        FE_GRAD_CASE(16, dbg_geo)    // temporal loads
        FE_GRAD_CASE(20, dbg_geo)    // both
        case 32:                     // per-wave time stamps, of the dynamic walk too (one field)
            if (gsec)
                return mfma_launch<fe::grad3d_mfma_kernel<NP, M, 32, true, true>>(
                    s, walk_static(nTiles), stamps_geo, "experiment",
                    [&](const Launch&) { return call(opT, 0, P, D, gsec, nb, nx, E, nTiles, opT); });
            return mfma_launch<fe::grad3d_mfma_kernel<NP, M, 32>, fe::grad3d_mfma_tail_kernel<NP, M, 32>>(
                s, walk_tickets(nTiles, nb == 1), stamps_geo, "experiment",
                [&](const Launch& L) {   // (as the product's static walk)
                    const int f = opT | (nb == 1 ? write_through_flag(3 * (int64_t)NP * E * 8) | grad_quarter_flag(M, nb, nTiles, L.waves()) : 0);
                    return call(f, 0, P, D, nullptr, nb, nx, E, nTiles, f);
                },
                "experiment", tail_args);
        FE_GRAD_CASE(64, dbg_geo)
        FE_GRAD_CASE(96, stamps_geo)
        FE_GRAD_CASE(128, dbg_geo)
        default: break;
    }
#undef FE_GRAD_CASE
#else
    (void)dbg;
#endif
    if (gsec) {
        snprintf(what, sizeof(what), "grad Np=%d M=%d, prepared operator", NP, M);
        return mfma_launch<fe::grad3d_mfma_kernel<NP, M, 0, true, true>>(
            s, walk_static(nTiles), geo, what, [&](const Launch&) { return call(opT, 0, P, D, gsec, nb, nx, E, nTiles, opT); });
    }
    // behind two static rounds the tiles come by tickets (fe_common.h: dynamic walk); any number of fields.  One field (a short
    // launch) writes through under either walk; under the static walk its ragged last round runs as quarter tiles and it starts
    // staggered (the rules: grad_quarter_flag, grad_stagger_flag)
    auto static_args = [&](const Launch& L) {
        const int f = opT | (nb == 1 ? write_through_flag(3 * (int64_t)NP * E * 8) | grad_quarter_flag(M, nb, nTiles, L.waves()) |
                                           grad_stagger_flag(NP, M, nb, nTiles, L.waves())
                                     : 0);
        return call(f, ((f & fe::kOpQuarterTail) ? 8 : 0) | ((f & fe::kOpStaggeredStart) ? 16 : 0), P, D, nullptr, nb, nx, E, nTiles, f);
    };
    snprintf(what, sizeof(what), "grad Np=%d M=%d", NP, M);
    if (nb == 1) {
        snprintf(tail_what, sizeof(tail_what), "grad Np=%d M=%d, dynamic walk", NP, M);
        const int f = opT | write_through_flag(3 * (int64_t)NP * E * 8);
        return mfma_launch<fe::grad3d_mfma_kernel<NP, M, 0>, fe::grad3d_mfma_tail_kernel<NP, M>>(
            s, walk_tickets(nTiles), geo, what, static_args, tail_what,
            [&](const Launch& L) { return call(f, 0, P, D, nb, E, nTiles, f, L.tail, L.t_static[0]); });
    }
    snprintf(tail_what, sizeof(tail_what), "grad Np=%d M=%d x b, dynamic walk", NP, M);
    return mfma_launch<fe::grad3d_mfma_kernel<NP, M, 0>, fe::grad3d_mfma_tail_kernel<NP, M, 0, true>>(
        s, walk_tickets(nTiles), geo, what, static_args, tail_what, tail_args);
}

template <int NP, int M>
int launch_div(const double* J, const double* D, const void* prep, const fe::FieldPtrs& P, int nb, int64_t E, int dbg,
               int opT, hipStream_t s, int64_t* e_done) {
    using G = fe::DivGeom<NP, M>;
    const int64_t nTiles = E / G::TEL;
    *e_done = nTiles > 0 ? E : 0;   // the launch covers the elements behind the last tile too (remainder_items)
    if (nTiles == 0) return FE_OK;
    opT |= temporal_flag((9 + 3 * (int64_t)nb * NP) * E * 8, kTemporalFloorDiv, kTemporalCapDivMib);
    const Geometry geo = {G::WAVES, 256, G::LDS_BYTES, G::BLOCKS_PER_CU, 8 / G::WAVES};
    char what[64], tail_what[64];
    // (recorded: the static walk's stores are never write-through)
    auto args = [&](const Launch&) { return call(opT & ~fe::kOpStoresWriteThrough, 0, J, D, nullptr, P, nb, E, nTiles, opT, 0); };
    auto tail_args = [&](const Launch& L) { return call(opT, 0, J, D, P, nb, E, nTiles, opT, L.tail, L.t_static[0]); };
#ifdef FE_EXPERIMENTS
    const Geometry dbg_geo = {G::WAVES, 256, G::LDS_BYTES, 1, 8 / G::WAVES},
                   stamps_geo = {G::WAVES, 256, G::LDS_BYTES + fe::kDbgTileLdsBytes, 1, 8 / G::WAVES};
#define FE_DIV_CASE(DBG) \
    case DBG: return mfma_launch<fe::div3d_mfma_kernel<NP, M, DBG>>(s, walk_static(nTiles), dbg_geo, "experiment", args);
    switch (NP == 35 ? dbg : 0) {
        FE_DIV_CASE(1)
        FE_DIV_CASE(2)
        FE_DIV_CASE(3)
        FE_DIV_CASE(8)
        FE_DIV_CASE(32)   // one u plane loaded instead of three (timing only)
        FE_DIV_CASE(64)   // the tile after next touched line by line (L2 prefetch)
        case 128:         // per-wave, per-tile time stamps (fe_dbg_tile); FE_DIV_ILV=1: of the interleaved kernel
            if constexpr (NP == 35 && M == 1) {
                if (getenv("FE_DIV_ILV"))
                    return mfma_launch<fe::div3d_mfma_ilv_kernel<NP, 128>>(
                        s, walk_static(nTiles), stamps_geo, "experiment",
                        [&](const Launch&) { return call(opT, 0, J, D, P, nb, E, nTiles, opT); });
            }
            return mfma_launch<fe::div3d_mfma_kernel<NP, M, 128>>(s, walk_static(nTiles), stamps_geo, "experiment", args);
        default: break;
    }
#undef FE_DIV_CASE
#else
    (void)dbg;
#endif
    if (prep) {
        snprintf(what, sizeof(what), "div Np=%d M=%d, prepared operator", NP, M);
        return mfma_launch<fe::div3d_mfma_kernel<NP, M, 0, 0, 3, false, false, true>>(
            s, walk_static(nTiles), geo, what,
            [&](const Launch&) { return call(opT & ~fe::kOpStoresWriteThrough, 0, J, D, prep, P, nb, E, nTiles, opT, 0); });
    }
    snprintf(what, sizeof(what), "div Np=%d M=%d", NP, M);
    // behind two static rounds the tiles come by tickets (fe_common.h); any number of fields -- not under the split walk
    const bool tickets = !(opT & fe::kDivWalkSplit);
    if constexpr (NP == 35 && M == 1) {
        const bool ilv = nTiles <= g_div_interleave_tiles.load(std::memory_order_relaxed);
        if (tickets && ilv && tail_static_tiles(nTiles, persistent_grid(nTiles, G::WAVES), G::WAVES) == nTiles) {
            // a short launch (static walk): the interleaved form, the ragged last round of one field as quarter tiles
            if (int rc = configured<fe::div3d_mfma_kernel<NP, M, 0>>(what, G::LDS_BYTES, 256, G::BLOCKS_PER_CU)) return rc;
            return mfma_launch<fe::div3d_mfma_ilv_kernel<NP>>(s, walk_static(nTiles), geo, "div Np=35, B build interleaved",
                                                              [&](const Launch& L) {
                const int64_t ragged = nTiles % L.waves();   // (the kernel's own rule: fe_div.h)
                const int q = (nb == 1 && ragged > 0 && 8 * ragged <= L.waves() && g_div_quarter_tail.load(std::memory_order_relaxed))
                                  ? fe::kOpQuarterTail : 0;
                return call(opT & ~fe::kOpStoresWriteThrough, 4 | (q ? 8 : 0), J, D, P, nb, E, nTiles, opT | q);
            });
        }
        if (nb == 1 && ilv)   // the interleaved form, dynamic walk
            return mfma_launch<fe::div3d_mfma_kernel<NP, M, 0>, fe::div3d_mfma_tail_kernel<NP, M, false, true>>(
                s, walk_tickets(nTiles, tickets), geo, what, args, "div Np=35, B build interleaved, dynamic walk",
                [&](const Launch& L) { return call(opT, 4, J, D, P, nb, E, nTiles, opT, L.tail, L.t_static[0]); });
    }
    if (nb == 1) {
        snprintf(tail_what, sizeof(tail_what), "div Np=%d M=%d, dynamic walk", NP, M);
        return mfma_launch<fe::div3d_mfma_kernel<NP, M, 0>, fe::div3d_mfma_tail_kernel<NP, M>>(
            s, walk_tickets(nTiles, tickets), geo, what, args, tail_what, tail_args);
    }
    snprintf(tail_what, sizeof(tail_what), "div Np=%d M=%d x b, dynamic walk", NP, M);
    return mfma_launch<fe::div3d_mfma_kernel<NP, M, 0>, fe::div3d_mfma_tail_kernel<NP, M, true>>(
        s, walk_tickets(nTiles, tickets), geo, what, args, tail_what, tail_args);
}

template <int NP, int M, bool ALDS = false>
int launch_divcomp(const double* J, const double* D, const double* u, double* out, int64_t E,
                   int opT, int jes, hipStream_t s, int64_t* e_done) {
    using G = fe::DivGeom<NP, M, 1, 3, ALDS>;
    const int64_t nTiles = E / G::TEL;
    *e_done = nTiles > 0 ? E : 0;   // the launch covers the elements behind the last tile too (remainder_items)
    if (nTiles == 0) return FE_OK;
    fe::FieldPtrs P = {};
    P.v[0] = u;
    P.out[0] = out;
    char what[64];
    snprintf(what, sizeof(what), "div component Np=%d M=%d", NP, M);
    // (the grid of 8 waves per CU, but no more blocks than are resident)
    const Geometry geo = {G::WAVES, 256, G::LDS_BYTES, G::BLOCKS_PER_CU, G::BLOCKS_PER_CU == 1 ? 1 : 8 / G::WAVES};
    return mfma_launch<fe::div3d_mfma_kernel<NP, M, 0, 1, 3, ALDS>>(
        s, walk_static(nTiles), geo, what, [&](const Launch&) { return call(opT, 0, J, D, nullptr, P, 1, E, nTiles, opT, jes); });
}

// 'e,ij,ej->ei' (MODE 2) / 'ij,ej->ei' (MODE 3): the one-component instances of the div template
template <int NP, int M, int MODE>
int launch_matapply_mode(const double* J, const double* D, const fe::FieldPtrs& P, int nb, int64_t E, int opT,
                         hipStream_t s, int64_t* e_done) {
    using G = fe::DivGeom<NP, M, MODE>;
    const int64_t nTiles = E / G::TEL;
    *e_done = nTiles > 0 ? E : 0;   // the launch covers the elements behind the last tile too (remainder_items)
    if (nTiles == 0) return FE_OK;
    char what[64];
    snprintf(what, sizeof(what), "matapply Np=%d M=%d mode %d", NP, M, MODE);
    return mfma_launch<fe::div3d_mfma_kernel<NP, M, 0, MODE>>(
        s, walk_static(nTiles), {G::WAVES, 256, G::LDS_BYTES, G::BLOCKS_PER_CU, 8 / G::WAVES}, what,
        [&](const Launch&) { return call(opT, 0, J, D, nullptr, P, nb, E, nTiles, opT, 0); });
}

template <int NP, int M>
int launch_matapply(const double* J, const double* D, const fe::FieldPtrs& P, int nb, int64_t E, int opT,
                    hipStream_t s, int64_t* e_done) {
    return J ? launch_matapply_mode<NP, M, 2>(J, D, P, nb, E, opT, s, e_done)
             : launch_matapply_mode<NP, M, 3>(J, D, P, nb, E, opT, s, e_done);
}

template <int NP, int NFP, int M, int NB, int NF = fe::kFmNf, bool ALDS = false>
int launch_fm_nb(const double* J, const double* R, const void* prep, const fe::FieldPtrs& P, int64_t E, int64_t nTiles,
                 int jfe, int rifj, hipStream_t s) {
    constexpr bool W8 = ALDS;   // fragments in LDS: eight waves per block share them, one block per CU
    using G = fe::FmGeom<NP, NFP, M, NF, ALDS, W8>;
    jfe = (jfe ? 1 : 0) | temporal_flag((NF + (int64_t)NB * NF * NFP) * E * 8, kTemporalFloorFaceMass, kTemporalCapFaceMassMib);
    const Geometry geo = {G::WAVES, G::THREADS, G::LDS_BYTES, G::BLOCKS_PER_CU, G::BLOCKS_PER_CU};
    char what[96], tail_what[96];
    if constexpr (!ALDS && NF == fe::kFmNf && NB >= 2) {   // prepared operators: tetrahedra p = 1..4, two or more fields
        if (prep) {
            snprintf(what, sizeof(what), "face-mass Np=%d Nfp=%d M=%d b=%d, prepared operator", NP, NFP, M, NB);
            return mfma_launch<fe::facemass_mfma_kernel<NP, NFP, M, NB, NF, false, false, true>>(
                s, walk_static(nTiles), geo, what,
                [&](const Launch&) { return call(jfe & ~fe::kOpStoresWriteThrough, 0, J, R, prep, P, E, nTiles, jfe, rifj); });
        }
    }
    snprintf(what, sizeof(what), "face-mass Np=%d Nfp=%d nf=%d M=%d b=%d", NP, NFP, NF, M, NB);
    auto args = [&](const Launch&) { return call(jfe & ~fe::kOpStoresWriteThrough, 0, J, R, nullptr, P, E, nTiles, jfe, rifj); };
    auto tail_args = [&](const Launch& L) { return call(jfe, 0, J, R, P, E, nTiles, jfe, rifj, L.tail, L.t_static[0]); };
    constexpr auto K = fe::facemass_mfma_kernel<NP, NFP, M, NB, NF, ALDS, W8>;
    // behind two static rounds the tiles come by tickets (fe_common.h, dynamic walk): p = 5 x 4, and tetrahedra p = 1 .. 4 and
    // triangles with three or more fields, or with one (from four and a half rounds on, as every single launch)
    if constexpr (NP == 56 && NFP == 21 && M == 1 && NF == fe::kFmNf && ALDS && NB == 4) {
        snprintf(tail_what, sizeof(tail_what), "face-mass Np=56 b=%d (A in LDS), dynamic walk", NB);
        return mfma_launch<K, fe::facemass_w8_tail_kernel<NP, NFP, NB>>(s, walk_tickets(nTiles), geo, what, args, tail_what, tail_args);
    } else if constexpr (!ALDS && NB == 1) {
        snprintf(tail_what, sizeof(tail_what), "face-mass Np=%d nf=%d M=%d b=1, dynamic walk", NP, NF, M);
        return mfma_launch<K, fe::facemass_mfma_tail_kernel<NP, NFP, M, 1, NF>>(s, walk_tickets(nTiles), geo, what, args, tail_what,
                                                                               tail_args);
    } else if constexpr (!ALDS && NB >= 3) {
        snprintf(tail_what, sizeof(tail_what), "face-mass Np=%d nf=%d M=%d b=%d, dynamic walk", NP, NF, M, NB);
        return mfma_launch<K, fe::facemass_mfma_tail_kernel<NP, NFP, M, NB, NF>>(
            s, walk_tickets(nTiles, true, NP == 35 && NF == fe::kFmNf && NB == 4), geo, what, args, tail_what, tail_args);
    } else {
        return mfma_launch<K>(s, walk_static(nTiles), geo, what, args);
    }
}

// One MFMA launch for a group of nb fields (nb <= kMaxGroup of the geometry; nb = 1 only for a call of one field).
template <int NP, int NFP, int M, int NF = fe::kFmNf, bool ALDS = false>
int launch_fm(const double* J, const double* R, const void* prep, const fe::FieldPtrs& P, int nb, int64_t E,
              int64_t nTiles, int jfe, int rifj, hipStream_t s) {
    int rc = FE_OK;
    auto launch = [&](auto NB) { return launch_fm_nb<NP, NFP, M, decltype(NB)::value, NF, ALDS>(J, R, prep, P, E, nTiles, jfe, rifj, s); };
    if (fe::with_field_count<1, 4>(nb, &rc, launch)) return rc;
    if constexpr (NP == 35 && NF == fe::kFmNf) {   // p = 4, the headline order: groups of up to 8 fields
        if (fe::with_field_count<5, 8>(nb, &rc, launch)) return rc;
    }
    return fail(FE_EINVAL, "face-mass: internal field grouping error (nb=%d)", nb);
}

// The accumulating face-mass launch (fe_facemass_acc_f64; fe_facemass.h, kAcc): static walk, the plain operator
template <int NP, int NFP, int M, int NB>
int launch_fm_acc_nb(const double* J, const double* R, const fe::FieldPtrs& P, int64_t E, int64_t nTiles, int jfe, int rifj,
                     double alpha, double beta, hipStream_t s) {
    using G = fe::FmGeom<NP, NFP, M>;
    // (with beta != 0 the launch reads its outputs too: they count as inputs for the cache rule)
    const int64_t in_doubles = fe::kFmNf + (int64_t)NB * fe::kFmNf * NFP + (beta != 0.0 ? (int64_t)NB * NP : 0);
    jfe = (jfe ? 1 : 0) | temporal_flag(in_doubles * E * 8, kTemporalFloorFaceMass, kTemporalCapFaceMassMib);
    char what[96];
    snprintf(what, sizeof(what), "face-mass Np=%d Nfp=%d M=%d b=%d, accumulating", NP, NFP, M, NB);
    return mfma_launch<fe::facemass_mfma_acc_kernel<NP, NFP, M, NB>>(
        s, walk_static(nTiles), {G::WAVES, G::THREADS, G::LDS_BYTES, G::BLOCKS_PER_CU, G::BLOCKS_PER_CU}, what,
        [&](const Launch&) { return call(jfe & ~fe::kOpStoresWriteThrough, 0, J, R, P, E, nTiles, jfe, rifj, alpha, beta); });
}

template <int NP, int NFP, int M>
int launch_fm_acc(const double* J, const double* R, const fe::FieldPtrs& P, int nb, int64_t E, int64_t nTiles, int jfe, int rifj,
                  double alpha, double beta, hipStream_t s) {
    int rc = FE_OK;
    if (fe::with_field_count<2, 4>(nb, &rc, [&](auto NB) {
            return launch_fm_acc_nb<NP, NFP, M, decltype(NB)::value>(J, R, P, E, nTiles, jfe, rifj, alpha, beta, s);
        }))
        return rc;
    return fail(FE_EINVAL, "accumulating face-mass: internal field grouping error (nb=%d)", nb);
}

// The accumulating grad and div launches (fe_grad3d_acc_f64, fe_div3d_acc_f64; fe_grad.h / fe_div.h, kAcc): one field, static
// walk, the plain operator, full tiles, non-temporal stores -- op_flags carries the operator layout and the temporal-load bit
// only (no write-through, quarter tiles, staggered start, split walk; the kernels compile those forms out anyway).
template <int NP, int M>
int launch_grad_acc(const fe::GradFields& P, const double* D, int64_t E, int opT, double alpha, double beta, hipStream_t s,
                    bool* launched) {
    using G = fe::GradGeom<NP, M>;
    const int64_t nTiles = E / G::TEL;   // full wave tiles; the launch covers the elements behind the last one too
    *launched = nTiles > 0;
    if (nTiles == 0) return FE_OK;
    // (with beta != 0 the launch reads its output too: it counts as an input for the cache rule)
    const int64_t in_doubles = 9 + (int64_t)NP + (beta != 0.0 ? 3 * (int64_t)NP : 0);
    const int f = (opT ? 1 : 0) | temporal_flag(in_doubles * E * 8);
    char what[96];
    snprintf(what, sizeof(what), "grad Np=%d M=%d, accumulating", NP, M);
    return mfma_launch<fe::grad3d_mfma_acc_kernel<NP, M>>(s, walk_static(nTiles), {G::WAVES, 256, G::LDS_BYTES, 2, 8 / G::WAVES}, what,
                                                          [&](const Launch&) { return call(f, 0, P, D, E, nTiles, f, alpha, beta); });
}

template <int NP, int M>
int launch_div_acc(const double* J, const double* D, const fe::FieldPtrs& P, int64_t E, int opT, double alpha, double beta,
                   hipStream_t s, bool* launched) {
    using G = fe::DivGeom<NP, M>;
    const int64_t nTiles = E / G::TEL;
    *launched = nTiles > 0;
    if (nTiles == 0) return FE_OK;
    const int64_t in_doubles = 9 + 3 * (int64_t)NP + (beta != 0.0 ? (int64_t)NP : 0);
    const int f = (opT ? 1 : 0) | temporal_flag(in_doubles * E * 8, kTemporalFloorDiv, kTemporalCapDivMib);
    char what[96];
    snprintf(what, sizeof(what), "div Np=%d M=%d, accumulating", NP, M);
    return mfma_launch<fe::div3d_mfma_acc_kernel<NP, M>>(
        s, walk_static(nTiles), {G::WAVES, 256, G::LDS_BYTES, G::BLOCKS_PER_CU, 8 / G::WAVES}, what,
        [&](const Launch&) { return call(f, 0, J, D, P, E, nTiles, f, alpha, beta); });
}

// The launches on element slices (fe_grad3d_strided_f64, fe_div3d_strided_f64, fe_facemass_strided_f64; kLd in fe_grad.h,
// fe_div.h, fe_facemass.h): E is the launch's element count -- tiles, grid, the footprint rules of the cache hints -- and the
// plane distances of the arrays are arguments of their own.  The plain operator, full tiles; no write-through, quarter
// tiles, staggered start, interleaved build or split walk (the kernels compile those forms out).  Walks as the contiguous
// launchers: behind two static rounds the tiles come by tickets (grad, div; face-mass of three or more fields).
template <int NP, int M>
int launch_grad_strided(const fe::GradFields& P, const double* D, int nb, int64_t E, int64_t ldJ, int64_t ldOut, int opT,
                        hipStream_t s, bool* launched) {
    using G = fe::GradGeom<NP, M>;
    const int64_t nTiles = E / G::TEL;   // full wave tiles; the launch covers the elements behind the last one too
    *launched = nTiles > 0;
    if (nTiles == 0) return FE_OK;
    const int f = (opT ? 1 : 0) | temporal_flag((9 + (int64_t)nb * NP) * E * 8);
    char what[96], tail_what[96];
    snprintf(what, sizeof(what), "grad Np=%d M=%d, element slice", NP, M);
    snprintf(tail_what, sizeof(tail_what), "grad Np=%d M=%d, element slice, dynamic walk", NP, M);
    // behind two static rounds the tiles come by tickets, as in launch_grad (fe_common.h: dynamic walk)
    return mfma_launch<fe::grad3d_mfma_strided_kernel<NP, M>, fe::grad3d_mfma_strided_tail_kernel<NP, M>>(
        s, walk_tickets(nTiles), {G::WAVES, 256, G::LDS_BYTES, 2, 8 / G::WAVES}, what,
        [&](const Launch&) { return call(f, 128, P, D, nb, E, ldJ, ldOut, nTiles, f); }, tail_what,
        [&](const Launch& L) { return call(f, 128, P, D, nb, E, ldJ, ldOut, nTiles, f, L.tail, L.t_static[0]); });
}

template <int NP, int M>
int launch_div_strided(const double* J, const double* D, const fe::FieldPtrs& P, int nb, int64_t E, int64_t ldJ, int64_t ldIn,
                       int opT, hipStream_t s, bool* launched) {
    using G = fe::DivGeom<NP, M>;
    const int64_t nTiles = E / G::TEL;
    *launched = nTiles > 0;
    if (nTiles == 0) return FE_OK;
    const int f = (opT ? 1 : 0) | temporal_flag((9 + 3 * (int64_t)nb * NP) * E * 8, kTemporalFloorDiv, kTemporalCapDivMib);
    char what[96], tail_what[96];
    snprintf(what, sizeof(what), "div Np=%d M=%d, element slice", NP, M);
    snprintf(tail_what, sizeof(tail_what), "div Np=%d M=%d, element slice, dynamic walk", NP, M);
    return mfma_launch<fe::div3d_mfma_strided_kernel<NP, M>, fe::div3d_mfma_strided_tail_kernel<NP, M>>(
        s, walk_tickets(nTiles), {G::WAVES, 256, G::LDS_BYTES, G::BLOCKS_PER_CU, 8 / G::WAVES}, what,
        [&](const Launch&) { return call(f, 128, J, D, P, nb, E, ldJ, ldIn, nTiles, f); }, tail_what,
        [&](const Launch& L) { return call(f, 128, J, D, P, nb, E, ldJ, ldIn, nTiles, f, L.tail, L.t_static[0]); });
}

template <int NP, int NFP, int M, int NB>
int launch_fm_strided_nb(const double* J, const double* R, const fe::FieldPtrs& P, int64_t E, int64_t ldJ, int64_t ldIn,
                         int64_t nTiles, int jfe, int rifj, hipStream_t s) {
    using G = fe::FmGeom<NP, NFP, M>;
    jfe = (jfe ? 1 : 0) | temporal_flag((fe::kFmNf + (int64_t)NB * fe::kFmNf * NFP) * E * 8, kTemporalFloorFaceMass, kTemporalCapFaceMassMib);
    char what[96], tail_what[96];
    snprintf(what, sizeof(what), "face-mass Np=%d Nfp=%d M=%d b=%d, element slice", NP, NFP, M, NB);
    const Geometry geo = {G::WAVES, G::THREADS, G::LDS_BYTES, G::BLOCKS_PER_CU, G::BLOCKS_PER_CU};
    auto args = [&](const Launch&) { return call(jfe, 128, J, R, P, E, ldJ, ldIn, nTiles, jfe, rifj); };
    if constexpr (NB >= 3) {   // three or more fields: the dynamic walk, as in launch_fm_nb
        snprintf(tail_what, sizeof(tail_what), "face-mass Np=%d M=%d b=%d, element slice, dynamic walk", NP, M, NB);
        return mfma_launch<fe::facemass_mfma_strided_kernel<NP, NFP, M, NB>, fe::facemass_mfma_strided_tail_kernel<NP, NFP, M, NB>>(
            s, walk_tickets(nTiles, true, NP == 35 && NB == 4), geo, what, args, tail_what,
            [&](const Launch& L) { return call(jfe, 128, J, R, P, E, ldJ, ldIn, nTiles, jfe, rifj, L.tail, L.t_static[0]); });
    } else {
        (void)tail_what;
        return mfma_launch<fe::facemass_mfma_strided_kernel<NP, NFP, M, NB>>(s, walk_static(nTiles), geo, what, args);
    }
}

template <int NP, int NFP, int M>
int launch_fm_strided(const double* J, const double* R, const fe::FieldPtrs& P, int nb, int64_t E, int64_t ldJ, int64_t ldIn,
                      int64_t nTiles, int jfe, int rifj, hipStream_t s) {
    int rc = FE_OK;
    if (fe::with_field_count<2, 4>(nb, &rc, [&](auto NB) {
            return launch_fm_strided_nb<NP, NFP, M, decltype(NB)::value>(J, R, P, E, ldJ, ldIn, nTiles, jfe, rifj, s);
        }))
        return rc;
    return fail(FE_EINVAL, "face-mass on an element slice: internal field grouping error (nb=%d)", nb);
}

// 'xre,rij,ej->xei' operands as grad-type planes: j[x] = J[x], out[k][x] = out_k[x]
fe::GradFields grad_fields(const double* J, const double* const* u, double* const* out, int nb, int64_t E,
                           int Np) {
    fe::GradFields P = {};
    for (int x = 0; x < 3; ++x) P.j[x] = J + (int64_t)x * 3 * E;
    for (int k = 0; k < nb; ++k) {
        P.u[k] = u[k];
        for (int x = 0; x < 3; ++x) P.out[k][x] = out[k] + (int64_t)x * E * Np;
    }
    return P;
}

// MFMA launch over the full tiles + generic kernels for the rest.  Jfull != nullptr: the planes
// are those of a plain grad (one [3][3][E] array, [3][E][Np] outputs).
int grad_fields_launch(const fe::GradFields& P, const double* Jfull, const double* D, const void* prep, int nb, int nx,
                       int64_t E, int Np, int opT, int variant, hipStream_t s) {
    const bool mfma_ok = fe::is_tet_order(Np) || (Np == 56 && Jfull);
    fe::FieldPtrs Pt = {};
    for (int k = 0; k < nb; ++k) { Pt.v[k] = P.u[k]; Pt.out[k] = P.out[k][0]; }
    const fe::TiledArgs ta = tiled_args(FE_FAMILY_GRAD, Jfull, D, Pt, nb, E, 3, Np, 0, 0, opT, 0, 0);
    KernelPath path;
    if (int rc = choose_path(variant >= 1000 ? FE_VARIANT_MFMA : variant, mfma_ok, Jfull && tiled_fits(ta), "grad", Np,
                             &path))
        return rc;
    if (path == kPathTiled) return launch_tiled(ta, s);
    if (path == kPathMfma && Np == 56) {   // p = 5: too many A fragments for the row-permuted kernel
        bool launched = false;
        int dbg5 = 0;
#ifdef FE_EXPERIMENTS
        if (variant >= 1000) dbg5 = (variant - 1000) & 127;   // experiment flags, see fe_div.h
#endif
        if (int rc = launch_grad_p5(Jfull, D, Pt, nb, E, opT, s, &launched, dbg5)) return rc;
        if (launched) {
            FE_HIP_CHECK(hipGetLastError());
            return FE_OK;
        }
        return tiled_fits(ta) ? launch_tiled(ta, s) : fail(FE_EUNSUPPORTED, "grad: no kernel for this size");
    }
    int64_t e_done = 0;
    if (path == kPathMfma) {
        int dbg = 0;
#ifdef FE_EXPERIMENTS
        if (variant >= 1000) dbg = (variant - 1000) & 255;   // experiment flags, see fe_grad.h
#endif
        if (int rc = fe::with_tet_order(Np, [&](auto o) {   // wave tile = 16 M elements
                using O = decltype(o);
                return launch_grad<O::NP, O::MG>(P, Jfull != nullptr, D, prep, nb, nx, E, dbg, opT, s, &e_done);
            }))
            return rc;
    }
    if (e_done < E) {
        const dim3 grid(generic_grid(E - e_done, Np)), block(256);
        for (int k = 0; k < nb; ++k) {
            if (Jfull) {
                hipLaunchKernelGGL(fe::grad3d_generic_kernel, grid, block, 0, s, Jfull, D, P.u[k], P.out[k][0], E,
                                   Np, e_done, opT);
                continue;
            }
            for (int x = 0; x < 3; ++x)
                if (P.out[k][x])
                    hipLaunchKernelGGL(fe::divcomp3d_generic_kernel, grid, block, 0, s, P.j[x], D, P.u[k],
                                       P.out[k][x], E, Np, e_done, opT, 0);
        }
    }
    FE_HIP_CHECK(hipGetLastError());
    return FE_OK;
}

// body order of the fused launches (fe_fused.h): chosen by measurement (tools/fused_order_ab.py)
constexpr int kFusedOrderGradDiv = 1;   // the younger half of the grid runs grad first: -1.5 ... -3.7 % in every placement
constexpr int kFusedOrderWaveOp = 3;    // the younger half runs grad, div, lift (rotating all three bodies by thirds of the grid cost time)

// div then grad in one persistent launch (full tiles only; e_done_* report what was covered)
template <int NP, int MG, int MD>
int launch_graddiv(const double* J, const double* D, const void* prep, const fe::GradFields& Pg,
                   const fe::FieldPtrs& Pd, int64_t E, hipStream_t s, int64_t* e_done_g, int64_t* e_done_d) {
    using GG = fe::GradGeom<NP, MG>;
    using GD = fe::DivGeom<NP, MD>;
    using G = fe::GradDivGeom<NP, MG, MD>;
    const int64_t nTilesG = E / GG::TEL, nTilesD = E / GD::TEL;
    *e_done_g = *e_done_d = (nTilesG > 0 || nTilesD > 0) ? E : 0;   // remainders included
    if (nTilesG == 0 && nTilesD == 0) return FE_OK;
    constexpr bool kDyn = NP == 35 && MG == 1 && MD == 1;   // bodies with a dynamic walk (fe_common.h)
    const Geometry geo = {4, 256, G::LDS_BYTES, 2, 2};
    const int loads = temporal_flag((9 + 4 * (int64_t)NP) * E * 8, 0, kTemporalCapGradDivMib);
    // body order (fe_fused.h): with the static walk the younger half of the grid runs grad first; with tickets every block
    // runs div, then grad (profiles/r03/dynamic_walk_fused.txt: 77.9 - 78.1 against 76.9 - 77.6 %)
    auto args = [&](const Launch& L) {
        int op_arg = ((L.tail ? 0 : kFusedOrderGradDiv) << 8) | loads;
#ifdef FE_EXPERIMENTS
        if (const char* o = getenv("FE_FUSED_ORDER")) op_arg = atoi(o) << 8;
#endif
        return call(op_arg & fe::kOpLoadsTemporal, 0, J, D, prep, Pg, Pd, E, nTilesG, nTilesD, op_arg,
                    fe::FusedTail{L.tail, L.t_static[0], L.t_static[1], 0});
    };
    char what[64];
    if (prep) {
        snprintf(what, sizeof(what), "div + grad Np=%d, prepared operator", NP);
        return mfma_launch<fe::graddiv3d_mfma_kernel<NP, MG, MD, true>>(s, {{nTilesD, nTilesG, 0}, 2, 0u, false}, geo, what, args);
    }
    snprintf(what, sizeof(what), "div + grad Np=%d", NP);
    constexpr auto K = fe::graddiv3d_mfma_kernel<NP, MG, MD, false, kDyn>;   // (takes the counters itself)
    return mfma_launch<K, (kDyn ? K : nullptr)>(s, {{nTilesD, nTilesG, 0}, 2, 3u, false}, geo, what, args, what, args);
}

// div, grad and face-mass x nb (2..4) in one persistent launch (full tiles only)
template <int NP, int NFP, int MG, int MD, int MF, int NB>
int launch_waveop_nb(const fe::WaveOpArgs& a, const fe::GradFields& Pg, const fe::FieldPtrs& Pd,
                     const fe::FieldPtrs& Pf, hipStream_t s) {
    using G = fe::WaveOpGeom<NP, NFP, MG, MD, MF>;
    constexpr bool kDyn = NP == 35 && NFP == 15 && MG == 1 && MD == 1 && MF == 1;   // bodies with a dynamic walk (fe_common.h)
    const Geometry geo = {4, 256, G::LDS_BYTES, 2, 2};
    const int loads = temporal_flag((9 + 4 * (int64_t)NP + 4 + (int64_t)NB * 4 * NFP) * a.E * 8, 0, kTemporalCapFaceMassMib);
    auto args = [&](const Launch& L) {
        fe::WaveOpArgs args = a;
        args.load_flags = loads;
        if (L.tail) args.order = 0;   // with tickets every block runs div, grad, lift (see launch_graddiv)
#ifdef FE_EXPERIMENTS
        if (const char* o = getenv("FE_FUSED_ORDER")) args.order = atoi(o);
#endif
        return call(loads & fe::kOpLoadsTemporal, 0, args, Pg, Pd, Pf, fe::FusedTail{L.tail, L.t_static[0], L.t_static[1], L.t_static[2]});
    };
    const Walk walk = {{a.nTilesD, a.nTilesG, a.nTilesF}, 3, NB >= 3 ? 7u : 3u, false};   // (the lift of two fields walks statically)
    char what[80];
    if (a.prepD && a.prepR) {
        snprintf(what, sizeof(what), "div + grad + face-mass Np=%d b=%d, prepared operators", NP, NB);
        return mfma_launch<fe::waveop3d_mfma_kernel<NP, NFP, MG, MD, MF, NB, true>>(s, walk, geo, what, args);
    }
    snprintf(what, sizeof(what), "div + grad + face-mass Np=%d b=%d", NP, NB);
    constexpr auto K = fe::waveop3d_mfma_kernel<NP, NFP, MG, MD, MF, NB, false, kDyn>;   // (takes the counters itself)
    return mfma_launch<K, (kDyn ? K : nullptr)>(s, walk, geo, what, args, what, args);
}

template <int NP, int NFP, int MG, int MD, int MF>
int launch_waveop(fe::WaveOpArgs a, const fe::GradFields& Pg, const fe::FieldPtrs& Pd, const fe::FieldPtrs& Pf,
                  int nb, hipStream_t s, bool* launched) {
    a.nTilesG = a.E / (16 * MG);
    a.nTilesD = a.E / (16 * MD);
    a.nTilesF = a.E / (16 * MF);
    a.order = kFusedOrderWaveOp;
#ifdef FE_EXPERIMENTS
    if (const char* o = getenv("FE_FUSED_ORDER")) a.order = atoi(o);
#endif
    *launched = a.nTilesG > 0 || a.nTilesD > 0 || a.nTilesF > 0;   // remainders included
    if (!*launched) return FE_OK;
    int rc = FE_OK;
    if (fe::with_field_count<2, 4>(nb, &rc, [&](auto NB) {
            return launch_waveop_nb<NP, NFP, MG, MD, MF, decltype(NB)::value>(a, Pg, Pd, Pf, s);
        }))
        return rc;
    return fail(FE_EINVAL, "waveop: internal field count error (nb=%d)", nb);
}

// triangles (ND = 2): grad by components (MODE 4) and div (MODE 0) instances of the div template
template <int NP, int M, int MODE>
int launch_nd2(const double* J, const double* D, const fe::FieldPtrs& P, int nb, int64_t E, int opT,
               hipStream_t s, bool* launched, int jes = 0) {
    using G = fe::DivGeom<NP, M, MODE, 2>;
    const int64_t nTiles = E / G::TEL;
    *launched = nTiles > 0;   // the launch covers the elements behind the last tile too
    if (nTiles == 0) return FE_OK;
    const Geometry geo = {G::WAVES, 256, G::LDS_BYTES, G::BLOCKS_PER_CU, 8 / G::WAVES};
    const char* kind = MODE == 4 ? "grad" : MODE == 1 ? "div component" : "div";
    char what[64], tail_what[64];
    snprintf(what, sizeof(what), "triangles %s Np=%d M=%d", kind, NP, M);
    auto args = [&](const Launch&) { return call(opT, 0, J, D, nullptr, P, nb, E, nTiles, opT, jes); };
    constexpr auto K = fe::div3d_mfma_kernel<NP, M, 0, MODE, 2>;
    if constexpr (MODE == 0 || MODE == 4) {   // behind two static rounds the tiles come by tickets (fe_common.h, dynamic walk)
        snprintf(tail_what, sizeof(tail_what), "triangles %s Np=%d M=%d, dynamic walk", kind, NP, M);
        return mfma_launch<K, fe::nd2_mfma_tail_kernel<NP, M, MODE>>(
            s, walk_tickets(nTiles), geo, what, args, tail_what,
            [&](const Launch& L) { return call(opT, 0, J, D, P, nb, E, nTiles, opT, L.tail, L.t_static[0]); });
    } else {
        return mfma_launch<K>(s, walk_static(nTiles), geo, what, args);
    }
}

template <int MODE>
int launch_nd2_np(const double* J, const double* D, const fe::FieldPtrs& P, int nb, int64_t E, int Np, int opT,
                  hipStream_t s, bool* launched, int jes = 0) {
    switch (Np) {   // triangles p = 1..5; a wave tile of 16 M elements moves a few KB
        case 21: return launch_nd2<21, (MODE == 0 ? 2 : 3), MODE>(J, D, P, nb, E, opT, s, launched, jes);
        case 15: return launch_nd2<15, 4, MODE>(J, D, P, nb, E, opT, s, launched, jes);
        case 10: return launch_nd2<10, 6, MODE>(J, D, P, nb, E, opT, s, launched, jes);
        case 6: return launch_nd2<6, 8, MODE>(J, D, P, nb, E, opT, s, launched, jes);
        default: return launch_nd2<3, 8, MODE>(J, D, P, nb, E, opT, s, launched, jes);
    }
}

// Fields `v[0 .. nb-1]` / `out[...]` of one launch, the unused slots padded with the first field
fe::FieldPtrs field_group(const double* const* v, double* const* out, int nb) {
    fe::FieldPtrs P;
    for (int k = 0; k < fe::kMaxFields; ++k) {
        P.v[k] = v[k < nb ? k : 0];
        P.out[k] = out[k < nb ? k : 0];
    }
    return P;
}

// float32 grad and div on the matrix cores (fe_grad_f32.h, fe_div_f32.h): one launch per field, every one on `s` (a dynamic walk
// uses the stream's counters in turn).  1: too few elements for a wave tile (the caller runs the tiled kernel).
template <typename G, auto K, auto KT = nullptr>
int launch_f32_fields(const fe_argpack* a, const double* const* vin, double* const* vout, int b, int flags, const char* what,
                      hipStream_t s) {
    const int64_t nTiles = a->E / G::TEL;
    if (nTiles == 0) return 1;
    const Geometry geo = {G::WAVES, 256, G::LDS_BYTES, G::BLOCKS_PER_CU, G::BLOCKS_PER_CU};
    const float* J = reinterpret_cast<const float*>(a->J);
    const float* D = reinterpret_cast<const float*>(a->D);
    for (int k = 0; k < b; ++k) {
        const float* u = reinterpret_cast<const float*>(vin[k]);
        float* out = reinterpret_cast<float*>(vout[k]);
        if (int rc = mfma_launch<K, KT>(
                s, walk_tickets(nTiles), geo, what, [&](const Launch&) { return call(flags, 0, J, D, u, out, a->E, nTiles, flags); },
                what, [&](const Launch& L) { return call(flags, 0, J, D, u, out, a->E, nTiles, flags, L.tail, L.t_static[0]); }))
            return rc;
    }
    FE_HIP_CHECK(hipGetLastError());
    return FE_OK;
}

// float32 face-mass x 4 (fe_facemass_f32.h): groups of up to kMaxFields fields share J and the fragments
template <typename G, auto K>
int launch_f32_facemass(const fe_argpack* a, const double* const* vin, double* const* vout, int b, int jl, int rl, const char* what,
                        hipStream_t s) {
    const int64_t nTiles = a->E / G::TEL;
    if (nTiles == 0) return 1;
    const Geometry geo = {G::WAVES, 256, G::LDS_BYTES, G::BLOCKS_PER_CU, G::BLOCKS_PER_CU};
    const float* J = reinterpret_cast<const float*>(a->J);
    const float* R = reinterpret_cast<const float*>(a->D);
    if (int rc = fe::for_each_field_group(b, fe::kMaxFields, false, [&](int k0, int nb) {
            const fe::FieldPtrs P = field_group(vin + k0, vout + k0, nb);
            return mfma_launch<K>(s, walk_static(nTiles), geo, what,
                                  [&](const Launch&) { return call(0, 0, J, R, P, nb, a->E, nTiles, jl, rl); });
        }))
        return rc;
    FE_HIP_CHECK(hipGetLastError());
    return FE_OK;
}

// ---- float32 fields in float64 grad, div and face-mass (fe_mixed.h).  A launch below one wave tile still runs one block: its
// remainder code covers every element.  `plain`: the launch's field loads go through registers (a field plane that does not
// start on an 8-byte boundary: fe_mixed.h).  grad and div take the same arguments: one launcher, one launch per field.
// Float32 results (OUT = float): `opT` also carries fe::kOpDwordStores, `kind` the bits that say so.
template <typename G, auto KD, auto KP, typename OUT = double>
int launch_mixed_fields(const double* J, const double* D, const float* const* v, OUT* const* outs, int b, int64_t E, int opT,
                     bool plain, const char* what, const char* what_plain, hipStream_t s, int kind = 0) {
    const int64_t nTiles = E / G::TEL;
    const Geometry geo = {G::WAVES, 256, G::LDS_BYTES, G::BLOCKS_PER_CU, G::BLOCKS_PER_CU};
    const Walk walk = walk_static(nTiles > 0 ? nTiles : 1);
    for (int k = 0; k < b; ++k) {
        const float* u = v[k];
        OUT* out = outs[k];
        auto args = [&](const Launch&) {
            return call(opT, fe::kLaunchMixedFields | (plain ? fe::kLaunchPlainFieldLoads : 0) | kind, J, D, u, out, E, nTiles, opT);
        };
        if (int rc = plain ? mfma_launch<KP>(s, walk, geo, what_plain, args) : mfma_launch<KD>(s, walk, geo, what, args)) return rc;
    }
    FE_HIP_CHECK(hipGetLastError());
    return FE_OK;
}

template <typename G, auto KD, auto KP>
int launch_mixed_facemass(const double* J, const double* R, const float* const* v, double* const* outs, int b, int64_t E, int jl,
                          int rl, bool plain, const char* what, const char* what_plain, hipStream_t s, int kind = 0) {
    const int64_t nTiles = E / G::TEL;
    const Geometry geo = {G::WAVES, 256, G::LDS_BYTES, G::BLOCKS_PER_CU, G::BLOCKS_PER_CU};
    const Walk walk = walk_static(nTiles > 0 ? nTiles : 1);
    // groups of up to kMaxFields fields share J and the fragments
    if (int rc = fe::for_each_field_group(b, fe::kMaxFields, false, [&](int k0, int nb) {
            const fe::FieldPtrs P = field_group(reinterpret_cast<const double* const*>(v) + k0, outs + k0, nb);
            auto args = [&](const Launch&) {
                return call(0, fe::kLaunchMixedFields | (plain ? fe::kLaunchPlainFieldLoads : 0) | kind, J, R, P, nb, E, nTiles, jl, rl);
            };
            return plain ? mfma_launch<KP>(s, walk, geo, what_plain, args) : mfma_launch<KD>(s, walk, geo, what, args);
        }))
        return rc;
    FE_HIP_CHECK(hipGetLastError());
    return FE_OK;
}

// A kernel's description (fe_kernel_resources), formatted once: a `static const What` per instantiation of a call site
struct What {
    char text[96];
    What(const char* fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(text, sizeof(text), fmt, ap);
        va_end(ap);
    }
    operator const char*() const { return text; }
};

// The field tables of an argument pack (fe_launch, fe_launch_f32): the b-field form (v / outs) when given, else the single
// pair (u / out).  `in` and `out` may point into the struct: filled in place, not copied.
struct PackFields {
    const void* one_in[1];
    double* one_out[1];
    const void* const* in;
    double* const* out;
    int b;
};
int pack_fields(const char* who, const fe_argpack* a, PackFields* f) {
    f->b = a->b > 0 ? a->b : 1;
    f->one_in[0] = a->u;
    f->one_out[0] = a->out;
    f->in = ptr_table(a->v);
    f->out = a->outs;
    if (!f->in || !f->out) {
        if (f->b != 1) return fail(FE_EINVAL, "%s: b = %d needs the v / outs pointer arrays", who, f->b);
        f->in = f->one_in;
        f->out = f->one_out;
    }
    return FE_OK;
}

// ---- prepared operators: what fe_prepare_operator wrote where (host-side record, so that a launcher
// can refuse a buffer prepared for another shape without reading device memory)
struct PreparedInfo { int kind, Np, nf, Nfp, flags; const void* op; int device; };   // op: the array it is a snapshot of
std::mutex g_prepared_mutex;
std::unordered_map<const void*, PreparedInfo> g_prepared;

// null: not usable (with *err set when the caller passed a buffer that does not fit the call)
const void* usable_prepared(const void* prepared, const void* op, int kind, int Np, int nf, int Nfp, int flags,
                            const char* what, int* err) {
    *err = FE_OK;
    if (!prepared) return nullptr;
    PreparedInfo info;
    {
        std::lock_guard<std::mutex> lock(g_prepared_mutex);
        auto it = g_prepared.find(prepared);
        if (it == g_prepared.end()) {
            *err = fail(FE_EINVAL, "%s: the prepared-operator buffer %p was not written by fe_prepare_operator in this "
                        "process", what, prepared);
            return nullptr;
        }
        info = it->second;
    }
    if (info.kind != kind || info.Np != Np || info.nf != nf || info.Nfp != Nfp || info.flags != flags) {
        *err = fail(FE_EINVAL, "%s: the prepared operator is for another call (kind %d Np %d nf %d Nfp %d flags %d; "
                    "this call: kind %d Np %d nf %d Nfp %d flags %d)", what, info.kind, info.Np, info.nf, info.Nfp,
                    info.flags, kind, Np, nf, Nfp, flags);
        return nullptr;
    }
    int dev = -1;
    (void)hipGetDevice(&dev);
    if (info.op != op || info.device != dev) {   // a snapshot of ANOTHER operator array of the same shape would compute silently with it
        *err = fail(FE_EINVAL, "%s: the prepared operator %p is a snapshot of the operator array %p on device %d, this call "
                    "passes the operator array %p on device %d", what, prepared, info.op, info.device, op, dev);
        return nullptr;
    }
    return prepared;
}
constexpr int kPreparedD = 1, kPreparedR = 2;   // D[3][Np][Np] (grad + div sections) / face-mass R

template <int NP, int MG, int MD>
void prepare_d(const double* D, void* prepared, int opT, hipStream_t s) {
    using GG = fe::GradGeom<NP, MG>;
    using GD = fe::DivGeom<NP, MD>;
    static_assert(fe::kPrepGradOff + ((GG::RT * GG::KS + 1) / 2) * 1024 <= fe::kPrepDivOff, "grad section");
    static_assert(fe::kPrepDivOff + ((GD::BT * GD::KSJ * GD::NC + 1) / 2) * 1024 <= fe::kPrepDivSmallOff, "div section");
    static_assert(fe::kPrepDivSmallOff + GD::ASMALL_D * 8 <= fe::kPreparedBytes, "div 4-row groups");
    hipLaunchKernelGGL((fe::grad_prepare_kernel<NP, MG>), dim3(GG::RT * GG::KS), dim3(64), 0, s, D, 
                       static_cast<char*>(prepared) + fe::kPrepGradOff, opT);
    hipLaunchKernelGGL((fe::div_prepare_kernel<NP, MD>), dim3(GD::BT * GD::KSJ * GD::NC + (GD::ASMALL_D + 63) / 64),
                       dim3(64), 0, s, D, prepared, opT);
}

template <int NP, int NFP, int M>
void prepare_r(const double* R, void* prepared, int rlayout, hipStream_t s) {
    using G = fe::FmGeom<NP, NFP, M>;
    static_assert(fe::kPrepFmOff + (((G::BT + G::NS) * G::KS + 1) / 2) * 1024 <= fe::kPreparedBytes, "face-mass section");
    hipLaunchKernelGGL((fe::facemass_prepare_kernel<NP, NFP, M>), dim3((G::BT + G::NS) * G::KS), dim3(64), 0, s, R,
                       prepared, rlayout);
}

struct FmChoice { int max_group, tel; };
// (Np, Nfp) pairs of tetrahedral orders p = 1..4 with nf = 4
inline bool fm_mfma_geometry(int Np, int nf, int Nfp, FmChoice* c) {
    if (nf == 3) {   // triangles p = 1..5
        if (Np == 21 && Nfp == 6) { *c = {4, 48}; return true; }
        if (Np == 15 && Nfp == 5) { *c = {4, 64}; return true; }
        if (Np == 10 && Nfp == 4) { *c = {4, 80}; return true; }
        if (Np == 6 && Nfp == 3) { *c = {4, 96}; return true; }
        if (Np == 3 && Nfp == 2) { *c = {4, 128}; return true; }
        return false;
    }
    if (nf != fe::kFmNf) return false;
    if (Np == 56 && Nfp == 21) { *c = {4, 16}; return true; }   // p = 5: A fragments in LDS
    if (!fe::is_tet_order(Np, Nfp)) return false;
    // (p = 4, the headline order: groups of up to 8 fields)
    *c = {Np == 35 ? 8 : 4, fe::with_tet_order(Np, [](auto o) { return 16 * decltype(o)::MF; })};
    return true;
}

// Index groups of a two-operand einsum for fe_einsum_contract, from the descriptor's strides alone: an output index
// carried by A and B (nonzero stride), or by neither (a broadcast), is batch; by A only m; by B only n; a summed index
// is k; an index of extent 1 adds nothing to any offset and is dropped (FE_CONTRACT_DROPPED).
void contract_groups(const fe_einsum_desc* d, int32_t* out_group, int32_t* sum_group) {
    for (int k = 0; k < d->n_out; ++k) {
        const bool a = d->op_out_stride[0][k] != 0, b = d->op_out_stride[1][k] != 0;
        out_group[k] = d->out_extent[k] == 1 ? FE_CONTRACT_DROPPED
                       : a == b              ? FE_CONTRACT_BATCH
                       : a                   ? FE_CONTRACT_M
                                             : FE_CONTRACT_N;
    }
    for (int k = 0; k < d->n_sum; ++k) sum_group[k] = d->sum_extent[k] == 1 ? FE_CONTRACT_DROPPED : FE_CONTRACT_K;
}

// The dtype field of an einsum descriptor: the compute type in the low byte, FE_DTYPE_OPERAND_F32 flags above it (float64
// compute only, operands < n_operands).  FE_OK with the flags in *f32_mask (bit p: operand p is float32).
int einsum_dtype(const char* who, const fe_einsum_desc* d, unsigned* f32_mask) {
    const unsigned bits = (unsigned)d->dtype, code = bits & 0xffu, flags = bits & ~0xffu;
    *f32_mask = 0;
    if (flags & ~(unsigned)FE_DTYPE_OPERAND_F32_MASK) return fail(FE_EINVAL, "%s: unknown dtype bits 0x%x", who, bits);
    if (flags) {
        if (code != FE_DTYPE_F64)
            return fail(FE_EINVAL, "%s: float32 operand flags need the float64 compute type (dtype 0x%x)", who, bits);
        if ((flags >> 8) >> d->n_operands)
            return fail(FE_EINVAL, "%s: float32 flag of a missing operand (dtype 0x%x, %d operands)", who, bits,
                        d->n_operands);
        *f32_mask = flags >> 8;
        return FE_OK;
    }
    if (code != FE_DTYPE_F64 && code != FE_DTYPE_F32)
        return fail(FE_EUNSUPPORTED, "%s: dtype code %d not compiled (float64 / float32 only)", who, d->dtype);
    return FE_OK;
}

// ---- split reductions (fe_einsum_reduce_plan / fe_einsum_reduce, fe_reduce.h) ----
// The plan depends on the descriptor alone -- never on the device, its CU count or a knob -- so that a result is
// bitwise reproducible on every device of the architecture.  The limits mirror feinsum_amd/reduction.py
// (REDUCE_MAX_OUT, REDUCE_MAX_TILES) and contraction.py (AUTO_MIN_*): the MFMA path is taken where "auto" would run
// the two-operand einsum on the contraction kernel and its grid has few tiles.
constexpr int64_t kReduceMaxOut = 4096;        // output entries per row
constexpr int64_t kReduceMaxTiles = 256;       // MFMA path: batch x m tiles x n tiles below this
constexpr int64_t kReduceValuBlocks = 2048;    // VALU: slices x output chunks aimed at (8 blocks of 256 on 256 CUs)
constexpr int64_t kReduceMinPerWalker = 16;    // VALU: summation points per walker and slice, at least
constexpr int64_t kReduceMfmaItems = 512;      // MFMA: tiles x k slices aimed at (the persistent grid of 256 CUs)
constexpr int64_t kReduceMinKSteps = 8;        // MFMA: k steps of kCtBK per slice, at least
constexpr size_t kReduceWsAlign = 256;

struct SplitK {   // split-K launch of contract_launch: slices of slice_len k each, partials into ws
    int64_t slices, slice_len;
    void* ws;
};

struct AccScale {   // out <- alpha E + beta out (fe_einsum_contract_acc, fe_einsum_reduce_acc)
    double alpha, beta;
};

struct ReduceSetup {
    int path;               // FE_REDUCE_VALU / FE_REDUCE_MFMA
    int64_t n_out, slices;
    size_t ws_bytes, esize;
    unsigned f32_mask;
    int64_t k_slice_len;    // MFMA
    int64_t out_chunks;     // VALU
    fe::ReducePlan V;       // VALU
};

int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

int reduce_setup(const char* who, const fe_einsum_desc* d, ReduceSetup* r) {
    if (!d) return fail(FE_EINVAL, "%s: null descriptor", who);
    if (d->n_operands < 1 || d->n_operands > FE_MAX_EINSUM_OPERANDS || d->n_out < 0 ||
        d->n_out > FE_MAX_EINSUM_INDICES || d->n_sum < 0 || d->n_sum > FE_MAX_EINSUM_INDICES)
        return fail(FE_EINVAL, "%s: %d operands / %d output / %d summation indices out of range", who, d->n_operands,
                    d->n_out, d->n_sum);
    memset(r, 0, sizeof(*r));
    if (int rc = einsum_dtype(who, d, &r->f32_mask)) return rc;
    const bool f64 = (d->dtype & 0xff) == FE_DTYPE_F64;
    r->esize = f64 ? 8 : 4;
    int64_t n_out = 1, n_sum = 1;
    for (int k = 0; k < d->n_out; ++k) {
        if (d->out_extent[k] < 0) return fail(FE_EINVAL, "%s: negative extent", who);
        n_out *= d->out_extent[k];
    }
    for (int k = 0; k < d->n_sum; ++k) {
        if (d->sum_extent[k] < 0) return fail(FE_EINVAL, "%s: negative extent", who);
        n_sum *= d->sum_extent[k];
    }
    r->n_out = n_out;
    r->path = FE_REDUCE_VALU;
    if (n_out == 0) return FE_OK;   // nothing to launch, no workspace
    if (n_out > kReduceMaxOut)
        return fail(FE_EUNSUPPORTED, "%s: %lld output entries; a split reduction writes at most %lld", who,
                    (long long)n_out, (long long)kReduceMaxOut);

    if (d->n_operands == 2) {   // the contraction's groups (contract_groups) and the "auto" sizes
        int32_t og[FE_MAX_EINSUM_INDICES], sg[FE_MAX_EINSUM_INDICES];
        contract_groups(d, og, sg);
        int64_t M = 1, N = 1, B = 1, K = 1;
        for (int k = 0; k < d->n_out; ++k) {
            if (og[k] == FE_CONTRACT_M) M *= d->out_extent[k];
            else if (og[k] == FE_CONTRACT_N) N *= d->out_extent[k];
            else if (og[k] == FE_CONTRACT_BATCH) B *= d->out_extent[k];
        }
        for (int k = 0; k < d->n_sum; ++k) K *= d->sum_extent[k];
        const int64_t tiles = B * ceil_div(M, fe::kCtBM) * ceil_div(N, fe::kCtBM);
        if (M >= 16 && N >= 8 && K >= 8 && M * N >= 512 && tiles < kReduceMaxTiles) {
            int64_t S = std::min(ceil_div(kReduceMfmaItems, tiles), ceil_div(K, kReduceMinKSteps * fe::kCtBK));
            S = std::max<int64_t>(S, 1);
            r->k_slice_len = ceil_div(ceil_div(K, S), fe::kCtBK) * fe::kCtBK;
            r->path = FE_REDUCE_MFMA;
            r->slices = ceil_div(K, r->k_slice_len);
            r->ws_bytes = (size_t)ceil_div((int64_t)(r->slices * n_out * r->esize), kReduceWsAlign) * kReduceWsAlign;
            return FE_OK;
        }
    }

    // VALU: summation indices of extent 1 dropped, neighbours contiguous in every operand merged (outermost first)
    fe::ReducePlan& P = r->V;
    P.n_ops = d->n_operands;
    P.f32_mask = r->f32_mask;
    for (int k = 0; k < d->n_out; ++k) {
        if (d->out_extent[k] == 1) continue;
        P.out_ext[P.n_out] = d->out_extent[k];
        for (int p = 0; p < d->n_operands; ++p) P.out_st[p][P.n_out] = d->op_out_stride[p][k];
        ++P.n_out;
    }
    if (n_sum > 0)
        for (int k = 0; k < d->n_sum; ++k) {
            if (d->sum_extent[k] == 1) continue;
            bool merge = P.n_sum > 0;
            for (int p = 0; p < d->n_operands && merge; ++p)
                merge = P.sum_st[p][P.n_sum - 1] == d->op_sum_stride[p][k] * d->sum_extent[k];
            if (merge) {
                P.sum_ext[P.n_sum - 1] *= d->sum_extent[k];
                for (int p = 0; p < d->n_operands; ++p) P.sum_st[p][P.n_sum - 1] = d->op_sum_stride[p][k];
                continue;
            }
            P.sum_ext[P.n_sum] = d->sum_extent[k];
            for (int p = 0; p < d->n_operands; ++p) P.sum_st[p][P.n_sum] = d->op_sum_stride[p][k];
            ++P.n_sum;
        }
    P.n_out_entries = n_out;
    P.n_sum_points = n_sum;
    // lanes along the output when the largest operand's unit stride is an output index and no summation index
    int big = 0;
    double big_n = -1;
    for (int p = 0; p < d->n_operands; ++p) {
        double nel = 1;
        for (int k = 0; k < P.n_out; ++k) if (P.out_st[p][k]) nel *= (double)P.out_ext[k];
        for (int k = 0; k < P.n_sum; ++k) if (P.sum_st[p][k]) nel *= (double)P.sum_ext[k];
        if (nel > big_n) big = p, big_n = nel;
    }
    bool out_unit = false, sum_unit = false;
    for (int k = 0; k < P.n_out; ++k) out_unit |= std::abs(P.out_st[big][k]) == 1;
    for (int k = 0; k < P.n_sum; ++k) sum_unit |= std::abs(P.sum_st[big][k]) == 1;
    P.C = (out_unit && !sum_unit) ? (int32_t)std::min<int64_t>(n_out, fe::kRdThreads) : 1;
    P.R = fe::kRdThreads / P.C;
    P.R2 = 1;
    while (P.R2 < P.R) P.R2 *= 2;
    r->out_chunks = ceil_div(n_out, P.C);
    int64_t S = std::min(ceil_div(kReduceValuBlocks, r->out_chunks), ceil_div(n_sum, kReduceMinPerWalker * P.R));
    S = std::max<int64_t>(S, 1);
    P.slice_len = ceil_div(ceil_div(n_sum, S), 4) * 4;   // (a multiple of every vector width)
    P.slices = n_sum > 0 ? ceil_div(n_sum, P.slice_len) : 1;
    // one step of R points as digits of the summation space, and the offsets they and each wrap add
    int64_t rem = P.R;
    for (int t = 0; t < P.n_sum; ++t) {
        const int k = P.n_sum - 1 - t;
        P.step_dig[t] = k > 0 ? rem % P.sum_ext[k] : rem;
        rem = k > 0 ? rem / P.sum_ext[k] : 0;
        for (int p = 0; p < d->n_operands; ++p) {
            P.step_off[p] += P.step_dig[t] * P.sum_st[p][k];
            if (k > 0) P.wrap_off[p][k] = P.sum_st[p][k - 1] - P.sum_ext[k] * P.sum_st[p][k];
        }
    }
    r->slices = P.slices;
    r->ws_bytes = (size_t)ceil_div((int64_t)(r->slices * n_out * r->esize), kReduceWsAlign) * kReduceWsAlign;
    return FE_OK;
}

}  // namespace

extern "C" {

int fe_version(void) { return 1000; }

const char* fe_last_error(void) { return g_err; }

int fe_device_count(void) {
    int n = 0;
    FE_HIP_CHECK(hipGetDeviceCount(&n));
    return n;
}

int fe_device_info(int dev, char* name, size_t name_len, double* peak_f64_gflops,
                   double* peak_gbps) {
    hipDeviceProp_t p;
    FE_HIP_CHECK(hipGetDeviceProperties(&p, dev));
    const bool gfx950 = strstr(p.gcnArchName, "gfx950") != nullptr;
    if (name && name_len) {
        // ROCm often reports a generic marketing name ("AMD Radeon Graphics") or none at
        // all; the roofline tables are keyed by part, so gfx950 is named canonically.
        const char* nm = gfx950 ? "AMD Instinct MI355X" : (p.name[0] != 0 ? p.name : p.gcnArchName);
        strncpy(name, nm, name_len - 1);
        name[name_len - 1] = 0;
    }
    // fp64: vector = matrix = 32 FMA-flop/clk/SIMD.. i.e. 128 flop/clk/CU (MI355X: 256 CUs
    // x 2.4 GHz -> 78.6 TFLOP/s); HBM3E 8 TB/s (datasheet).  gfx950 only.
    const bool mi355 = gfx950;
    if (peak_f64_gflops)
        *peak_f64_gflops = mi355 ? 128.0 * p.multiProcessorCount * (p.clockRate * 1e-6) : 0.0;
    if (peak_gbps) *peak_gbps = mi355 ? 8000.0 : 0.0;
    return FE_OK;
}

int fe_prepare_operator(int32_t family, const double* op, int32_t Np, int32_t nf, int32_t Nfp, int32_t flags,
                        void* prepared, void* stream) {
    if (!op || !prepared) return fail(FE_EINVAL, "prepare: null pointer");
    if ((reinterpret_cast<uintptr_t>(op) & 7u) || (reinterpret_cast<uintptr_t>(prepared) & 15u))
        return fail(FE_EINVAL, "prepare: the operator must be 8-byte and the prepared buffer 16-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    PreparedInfo info{0, Np, 0, 0, flags, op, -1};
    (void)hipGetDevice(&info.device);
    if (family == FE_FAMILY_GRAD || family == FE_FAMILY_DIV || family == FE_FAMILY_GRADDIV) {
        if (flags & ~FE_OP_TRANSPOSED) return fail(FE_EINVAL, "prepare: bad operator flags %d", flags);
        const int opT = (flags & FE_OP_TRANSPOSED) ? 1 : 0;
        info.kind = kPreparedD;
        if (!fe::is_tet_order(Np)) return fail(FE_EUNSUPPORTED, "prepare: grad / div operators of tetrahedra p = 1..4 only (Np=%d)", Np);
        fe::with_tet_order(Np, [&](auto o) {
            using O = decltype(o);
            prepare_d<O::NP, O::MG, O::MD>(op, prepared, opT, s);
            return 0;
        });
    } else if (family == FE_FAMILY_FACEMASS) {
        if (flags & ~(FE_FM_R_IFJ | FE_FM_R_T)) return fail(FE_EINVAL, "prepare: bad face-mass operator flags %d", flags);
        const int rlayout = ((flags & FE_FM_R_IFJ) ? 1 : 0) + ((flags & FE_FM_R_T) ? 2 : 0);
        info.kind = kPreparedR;
        info.nf = nf;
        info.Nfp = Nfp;
        if (nf != fe::kFmNf) return fail(FE_EUNSUPPORTED, "prepare: face-mass operators of tetrahedra only (nf=%d)", nf);
        if (!fe::is_tet_order(Np, Nfp))
            return fail(FE_EUNSUPPORTED, "prepare: face-mass operators of tetrahedra p = 1..4 only (Np=%d Nfp=%d)", Np, Nfp);
        fe::with_tet_order(Np, [&](auto o) {
            using O = decltype(o);
            prepare_r<O::NP, O::NFP, O::MF>(op, prepared, rlayout, s);
            return 0;
        });
    } else {
        return fail(FE_EUNSUPPORTED, "prepare: family %d has no prepared form", family);
    }
    FE_HIP_CHECK(hipGetLastError());
    std::lock_guard<std::mutex> lock(g_prepared_mutex);
    g_prepared[prepared] = info;
    return FE_OK;
}

int fe_release_prepared(const void* prepared) {
    std::lock_guard<std::mutex> lock(g_prepared_mutex);
    return g_prepared.erase(prepared) ? FE_OK : fail(FE_EINVAL, "fe_release_prepared: %p is not a prepared-operator buffer of this process", prepared);
}

int fe_split_alloc(void** ptr, size_t bytes, int32_t flags) {
    SplitPool* pool = split_pool_of_current_device();
    std::lock_guard<std::mutex> lock(pool->mu);
    return pool->alloc(ptr, bytes, flags);
}

int fe_split_free(void* ptr) {
    if (!ptr) return FE_OK;
    const int dev = split_owner_device(ptr);
    if (dev < 0) return fail(FE_EINVAL, "fe_split_free: %p is not an array of the split allocator (on any device)", ptr);
    SplitDeviceScope scope(dev);
    SplitPool* pool = &g_split_pools[dev];
    std::lock_guard<std::mutex> lock(pool->mu);
    return pool->free_array(ptr);
}

int fe_split_info(const void* ptr, char* buf, size_t buf_len) {
    if (!buf || buf_len == 0) return fail(FE_EINVAL, "fe_split_info: no buffer");
    const int dev = split_owner_device(ptr);
    if (dev < 0) return fail(FE_EINVAL, "fe_split_info: %p is not an array of the split allocator (on any device)", ptr);
    SplitPool* pool = &g_split_pools[dev];
    std::lock_guard<std::mutex> lock(pool->mu);
    return pool->info(ptr, buf, buf_len);
}

int fe_split_stats(char* buf, size_t buf_len) {
    if (!buf || buf_len == 0) return fail(FE_EINVAL, "fe_split_stats: no buffer");
    SplitPool* pool = split_pool_of_current_device();
    std::lock_guard<std::mutex> lock(pool->mu);
    return pool->stats(buf, buf_len);
}

int fe_split_reserve(size_t bytes) {
    SplitPool* pool = split_pool_of_current_device();
    std::lock_guard<std::mutex> lock(pool->mu);
    return pool->reserve(bytes);
}

int fe_split_trim(void) {
    SplitPool* pool = split_pool_of_current_device();
    std::lock_guard<std::mutex> lock(pool->mu);
    return pool->trim();
}

int fe_kernel_resources(char* buf, size_t buf_len) {
    if (!buf || buf_len == 0) return fail(FE_EINVAL, "fe_kernel_resources: no buffer");
    std::lock_guard<std::mutex> lock(g_resources_mutex);
    strncpy(buf, g_resources.c_str(), buf_len - 1);
    buf[buf_len - 1] = 0;
    return (int)g_resources.size();
}

int64_t fe_flops_per_element(int32_t family, int32_t Np, int32_t nf, int32_t Nfp, int32_t b) {
    const int64_t np = Np;
    switch (family) {
        case FE_FAMILY_GRAD:
        case FE_FAMILY_DIV: return 2 * 3 * np * np + 2 * 9 * np;
        case FE_FAMILY_GRADDIV: return 2 * (2 * 3 * np * np + 2 * 9 * np);
        case FE_FAMILY_FACEMASS: return (int64_t)b * ((int64_t)nf * Nfp + 2 * np * nf * Nfp);
        case FE_FAMILY_DIVCOMP: return 3 * np + 2 * 3 * np * np;
        case FE_FAMILY_GRADPLANES: return (int64_t)(b > 0 ? b : 1) * (3 * np + 2 * 3 * np * np);   // b = output planes
        case FE_FAMILY_MATAPPLY: return (int64_t)(b > 0 ? b : 1) * (2 * np * np + np);                // with the J[e] factor
        default: return -1;
    }
}

int fe_grad3d_f64(const double* J, const double* D, const double* u, double* out, int64_t E,
                  int32_t Np, int32_t variant, void* stream) {
    return fe_grad3d_f64_ex(J, D, u, out, E, Np, 0, variant, stream);
}

int fe_grad3d_f64_ex(const double* J, const double* D, const double* u, double* out, int64_t E,
                     int32_t Np, int32_t op_flags, int32_t variant, void* stream) {
    return fe_grad3d_batched_f64(J, D, &u, &out, E, Np, 1, op_flags, variant, stream);
}

int fe_grad3d_batched_f64(const double* J, const double* D, const double* const* u,
                          double* const* out, int64_t E, int32_t Np, int32_t b, int32_t op_flags,
                          int32_t variant, void* stream) {
    return fe_grad3d_prepared_f64(J, D, nullptr, u, out, E, Np, b, op_flags, variant, stream);
}

int fe_grad3d_prepared_f64(const double* J, const double* D, const void* D_prepared, const double* const* u,
                           double* const* out, int64_t E, int32_t Np, int32_t b, int32_t op_flags,
                           int32_t variant, void* stream) {
    forget_last_launch();
    if (!u || !out) return fail(FE_EINVAL, "grad: null pointer table");
    if (b < 1) return fail(FE_EINVAL, "grad: b=%d, need at least one field", b);
    if (b > FE_MAX_FIELDS)   // FE_MAX_FIELDS fields per launch
        return fe::for_each_field_group(b, FE_MAX_FIELDS, false, [&](int k0, int nb) {
            return fe_grad3d_prepared_f64(J, D, D_prepared, u + k0, out + k0, E, Np, nb, op_flags, variant, stream);
        });
    int perr;
    const void* prep = usable_prepared(D_prepared, D, kPreparedD, Np, 0, 0, op_flags, "grad", &perr);
    if (perr != FE_OK) return perr;
    for (int k = 0; k < b; ++k)
        if (int rc = check_common("grad", J, D, u[k], out[k], E, Np)) return rc;
    if (op_flags & ~FE_OP_TRANSPOSED) return fail(FE_EINVAL, "grad: bad operator flags %d", op_flags);
    const int opT = (op_flags & FE_OP_TRANSPOSED) ? 1 : 0;
#ifdef FE_EXPERIMENTS
    if (variant < FE_VARIANT_AUTO || (variant > FE_VARIANT_TILED && variant < 1000))
#else
    if (variant < FE_VARIANT_AUTO || variant > FE_VARIANT_TILED)
#endif
        return fail(FE_EUNSUPPORTED, "grad: unknown variant %d", variant);
    if (E == 0) return FE_OK;
    return grad_fields_launch(grad_fields(J, u, out, b, E, Np), J, D, prep, b, 3, E, Np, opT, variant,
                              static_cast<hipStream_t>(stream));
}

int fe_gradplanes3d_f64(const double* const* J3, const double* D, const double* const* u,
                        double* const* out, int64_t E, int32_t Np, int32_t b, int32_t op_flags,
                        int32_t variant, void* stream) {
    forget_last_launch();
    if (!J3 || !u || !out) return fail(FE_EINVAL, "grad planes: null pointer table");
    if (b < 1) return fail(FE_EINVAL, "grad planes: b=%d, need at least one field", b);
    if (b > FE_MAX_FIELDS)   // FE_MAX_FIELDS fields per launch
        return fe::for_each_field_group(b, FE_MAX_FIELDS, false, [&](int k0, int nb) {
            return fe_gradplanes3d_f64(J3, D, u + k0, out + 3 * k0, E, Np, nb, op_flags, variant, stream);
        });
    if (op_flags & ~FE_OP_TRANSPOSED) return fail(FE_EINVAL, "grad planes: bad operator flags %d", op_flags);
    if (variant < FE_VARIANT_AUTO || variant > FE_VARIANT_TILED)
        return fail(FE_EUNSUPPORTED, "grad planes: unknown variant %d", variant);
    if (E < 0) return fail(FE_EINVAL, "grad planes: E must be >= 0 (got %lld)", (long long)E);
    if (E == 0) return FE_OK;   // empty arrays have no addresses to tell wanted planes from unwanted ones
    fe::GradFields P = {};
    int nx = -1;
    for (int k = 0; k < b; ++k) {
        int planes = 0;
        for (int x = 0; x < 3; ++x) {
            double* o = out[3 * k + x];
            if (!o) continue;
            if (int rc = check_common("grad planes", J3[x], D, u[k], o, E, Np)) return rc;
            P.out[k][x] = o;
            ++planes;
        }
        if (planes == 0) return fail(FE_EINVAL, "grad planes: field %d has no output plane", k);
        if (nx >= 0 && planes != nx)
            return fail(FE_EINVAL, "grad planes: every field of a call needs the same number of planes (%d vs %d)",
                        planes, nx);
        nx = planes;
        P.u[k] = u[k];
    }
    for (int x = 0; x < 3; ++x) {
        if (!J3[x]) return fail(FE_EINVAL, "grad planes: null geometry-factor array %d", x);
        if (reinterpret_cast<uintptr_t>(J3[x]) & 7u) return fail(FE_EINVAL, "grad planes: device pointers must be 8-byte aligned");
        P.j[x] = J3[x];
    }
    // The planes kernel is the row-permuted MFMA grad kernel (tetrahedra p = 1..4).  Whatever it does
    // not serve -- another order, or an explicitly requested tiled / generic variant -- runs plane by
    // plane through the div-component launcher, which has its own MFMA (p = 5), tiled and generic paths.
    const bool planes_kernel = fe::is_tet_order(Np) &&
                               (variant == FE_VARIANT_AUTO || variant == FE_VARIANT_MFMA);
    if (Np == 56 && (variant == FE_VARIANT_AUTO || variant == FE_VARIANT_MFMA)) {   // p = 5: grad by components
        bool launched = false;
        if (int rc = launch_gradplanes_p5(P, D, b, E, (op_flags & FE_OP_TRANSPOSED) ? 1 : 0, static_cast<hipStream_t>(stream),
                                          &launched))
            return rc;
        if (launched) {
            FE_HIP_CHECK(hipGetLastError());
            return FE_OK;
        }
    }
    if (!planes_kernel) {
        for (int k = 0; k < b; ++k)
            for (int x = 0; x < 3; ++x)
                if (P.out[k][x])
                    if (int rc = fe_divcomp3d_f64(P.j[x], D, P.u[k], P.out[k][x], E, Np, op_flags & FE_OP_TRANSPOSED,
                                                  variant, stream))
                        return rc;
        return FE_OK;
    }
    return grad_fields_launch(P, nullptr, D, nullptr, b, nx, E, Np, (op_flags & FE_OP_TRANSPOSED) ? 1 : 0, variant,
                              static_cast<hipStream_t>(stream));
}

int fe_div3d_f64(const double* J, const double* D, const double* u, double* out, int64_t E,
                 int32_t Np, int32_t variant, void* stream) {
    return fe_div3d_f64_ex(J, D, u, out, E, Np, 0, variant, stream);
}

int fe_div3d_f64_ex(const double* J, const double* D, const double* u, double* out, int64_t E,
                    int32_t Np, int32_t op_flags, int32_t variant, void* stream) {
    return fe_div3d_batched_f64(J, D, &u, &out, E, Np, 1, op_flags, variant, stream);
}

int fe_div3d_batched_f64(const double* J, const double* D, const double* const* u,
                         double* const* out, int64_t E, int32_t Np, int32_t b, int32_t op_flags,
                         int32_t variant, void* stream) {
    return fe_div3d_prepared_f64(J, D, nullptr, u, out, E, Np, b, op_flags, variant, stream);
}

int fe_div3d_prepared_f64(const double* J, const double* D, const void* D_prepared, const double* const* u,
                          double* const* out, int64_t E, int32_t Np, int32_t b, int32_t op_flags,
                          int32_t variant, void* stream) {
    forget_last_launch();
    if (!u || !out) return fail(FE_EINVAL, "div: null pointer table");
    if (b < 1) return fail(FE_EINVAL, "div: b=%d, need at least one field", b);
    if (b > FE_MAX_FIELDS)   // FE_MAX_FIELDS fields per launch
        return fe::for_each_field_group(b, FE_MAX_FIELDS, false, [&](int k0, int nb) {
            return fe_div3d_prepared_f64(J, D, D_prepared, u + k0, out + k0, E, Np, nb, op_flags, variant, stream);
        });
    int perr;
    const void* prep = usable_prepared(D_prepared, D, kPreparedD, Np, 0, 0, op_flags, "div", &perr);
    if (perr != FE_OK) return perr;
    fe::FieldPtrs P = {};
    for (int k = 0; k < b; ++k) {
        if (int rc = check_common("div", J, D, u[k], out[k], E, Np)) return rc;
        P.v[k] = u[k];
        P.out[k] = out[k];
    }
    if (op_flags & ~FE_OP_TRANSPOSED) return fail(FE_EINVAL, "div: bad operator flags %d", op_flags);
    const int opT = (op_flags & FE_OP_TRANSPOSED) ? 1 : 0;
#ifdef FE_EXPERIMENTS
    if (variant < FE_VARIANT_AUTO || (variant > FE_VARIANT_MFMA_SPLIT && variant < 1000))
#else
    if (variant < FE_VARIANT_AUTO || variant > FE_VARIANT_MFMA_SPLIT)
#endif
        return fail(FE_EUNSUPPORTED, "div: unknown variant %d", variant);
    if (E == 0) return FE_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool mfma_ok = Np == 56 || fe::is_tet_order(Np);
    const bool split_walk = variant == FE_VARIANT_MFMA_SPLIT;
    if (split_walk && !fe::is_tet_order(Np))
        return fail(FE_EUNSUPPORTED, "div: the split walk is a flavour of the p = 1..4 MFMA kernels (Np=%d)", Np);
    const fe::TiledArgs ta = tiled_args(FE_FAMILY_DIV, J, D, P, b, E, 3, Np, 0, 0, opT, 0, 0);
    KernelPath path;
    if (int rc = choose_path((variant >= 1000 || split_walk) ? FE_VARIANT_MFMA : variant, mfma_ok, tiled_fits(ta), "div", Np,
                             &path))
        return rc;
    if (path == kPathTiled) return launch_tiled(ta, s);
    if (path == kPathMfma && Np == 56) {   // p = 5
        bool launched = false;
        if (int rc = launch_div_p5(J, D, P, b, E, opT, s, &launched)) return rc;
        if (launched) {
            FE_HIP_CHECK(hipGetLastError());
            return FE_OK;
        }
        return tiled_fits(ta) ? launch_tiled(ta, s) : fail(FE_EUNSUPPORTED, "div: no kernel for this size");
    }
    int64_t e_done = 0;
    if (path == kPathMfma) {
        const int dbg = variant >= 1000 ? (variant - 1000) & 255 : 0;   // experiment builds only
        const int opf = opT | (split_walk ? fe::kDivWalkSplit : 0);
        if (int rc = fe::with_tet_order(Np, [&](auto o) {   // wave tile = 16 M elements
                using O = decltype(o);
                return launch_div<O::NP, O::MD>(J, D, prep, P, b, E, dbg, opf, s, &e_done);
            }))
            return rc;
    }
    if (e_done < E)
        for (int k = 0; k < b; ++k)
            hipLaunchKernelGGL(fe::div3d_generic_kernel, dim3(generic_grid(E - e_done, Np)), dim3(256),
                               0, s, J, D, P.v[k], P.out[k], E, Np, e_done, opT);
    FE_HIP_CHECK(hipGetLastError());
    return FE_OK;
}

// grad / div of ndim-dimensional elements: ndim = 3 is the 3d entry point; ndim = 2 (triangles)
// runs on the MFMA instances above for p = 1..5, else on the tiled kernel.
static int nd_launch(int family, const char* what, const double* J, const double* D, const double* const* u,
                     double* const* out, int64_t E, int32_t ndim, int32_t Np, int32_t b, int32_t op_flags,
                     int32_t variant, void* stream) {
    if (ndim != 2) return fail(FE_EUNSUPPORTED, "%s: ndim must be 2 or 3 (got %d)", what, ndim);
    if (!u || !out) return fail(FE_EINVAL, "%s: null pointer table", what);
    if (b < 1) return fail(FE_EINVAL, "%s: b=%d, need at least one field", what, b);
    if (op_flags & ~FE_OP_TRANSPOSED) return fail(FE_EINVAL, "%s: bad operator flags %d", what, op_flags);
    if (variant < FE_VARIANT_AUTO || variant > FE_VARIANT_TILED || variant == FE_VARIANT_GENERIC)
        return fail(FE_EUNSUPPORTED, "%s: ndim = 2 has the MFMA and the tiled kernels (variant %d)", what, variant);
    const bool mfma_ok = Np == 3 || Np == 6 || Np == 10 || Np == 15 || Np == 21;
    const int opT = (op_flags & FE_OP_TRANSPOSED) ? 1 : 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = fe::for_each_field_group(b, fe::kMaxFields, false, [&](int k0, int nb) {
            fe::FieldPtrs P = {};
            for (int k = 0; k < nb; ++k) {
                if (int rc = check_common(what, J, D, u[k0 + k], out[k0 + k], E, Np)) return rc;
                P.v[k] = u[k0 + k];
                P.out[k] = out[k0 + k];
            }
            if (E == 0) return FE_OK;
            const fe::TiledArgs ta = tiled_args(family, J, D, P, nb, E, ndim, Np, 0, 0, opT, 0, 0);
            KernelPath path;
            if (int rc = choose_path(variant, mfma_ok, tiled_fits(ta), what, Np, &path)) return rc;
            bool launched = false;
            if (path == kPathMfma) {
                const int rc = family == FE_FAMILY_GRAD ? launch_nd2_np<4>(J, D, P, nb, E, Np, opT, s, &launched)
                                                        : launch_nd2_np<0>(J, D, P, nb, E, Np, opT, s, &launched);
                if (rc != FE_OK) return rc;
            }
            if (!launched) {   // no MFMA geometry, or fewer elements than one wave tile
                if (!tiled_fits(ta)) return fail(FE_EUNSUPPORTED, "%s: no kernel for ndim = 2, Np = %d", what, Np);
                if (int rc = launch_tiled(ta, s)) return rc;
            }
            return FE_OK;
        }))
        return rc;
    FE_HIP_CHECK(hipGetLastError());
    return FE_OK;
}

int fe_grad_f64(const double* J, const double* D, const double* const* u, double* const* out, int64_t E,
                int32_t ndim, int32_t Np, int32_t b, int32_t op_flags, int32_t variant, void* stream) {
    forget_last_launch();
    if (ndim == 3) return fe_grad3d_batched_f64(J, D, u, out, E, Np, b, op_flags, variant, stream);
    return nd_launch(FE_FAMILY_GRAD, "grad", J, D, u, out, E, ndim, Np, b, op_flags, variant, stream);
}

int fe_div_f64(const double* J, const double* D, const double* const* u, double* const* out, int64_t E,
               int32_t ndim, int32_t Np, int32_t b, int32_t op_flags, int32_t variant, void* stream) {
    forget_last_launch();
    if (ndim == 3) return fe_div3d_batched_f64(J, D, u, out, E, Np, b, op_flags, variant, stream);
    return nd_launch(FE_FAMILY_DIV, "div", J, D, u, out, E, ndim, Np, b, op_flags, variant, stream);
}

int fe_divcomp_f64(const double* J, const double* D, const double* u, double* out, int64_t E, int32_t ndim,
                   int32_t Np, int32_t op_flags, int32_t variant, void* stream) {
    forget_last_launch();
    if (ndim == 3) return fe_divcomp3d_f64(J, D, u, out, E, Np, op_flags, variant, stream);
    if (ndim != 2) return fail(FE_EUNSUPPORTED, "div component: ndim must be 2 or 3 (got %d)", ndim);
    if (int rc = check_common("div component", J, D, u, out, E, Np)) return rc;
    if (op_flags & ~(FE_OP_TRANSPOSED | FE_OP_J_ES))
        return fail(FE_EINVAL, "div component: bad operator flags %d", op_flags);
    if (variant < FE_VARIANT_AUTO || variant > FE_VARIANT_TILED || variant == FE_VARIANT_GENERIC)
        return fail(FE_EUNSUPPORTED, "div component: ndim = 2 has the MFMA and the tiled kernels (variant %d)", variant);
    if (E == 0) return FE_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int opT = (op_flags & FE_OP_TRANSPOSED) ? 1 : 0, jes = (op_flags & FE_OP_J_ES) ? 1 : 0;
    const bool mfma_ok = Np == 3 || Np == 6 || Np == 10 || Np == 15 || Np == 21;
    fe::FieldPtrs P = {};
    P.v[0] = u;
    P.out[0] = out;
    const fe::TiledArgs ta = tiled_args(FE_FAMILY_DIVCOMP, J, D, P, 1, E, 2, Np, 0, 0, opT, jes, 0);
    KernelPath path;
    if (int rc = choose_path(variant, mfma_ok, tiled_fits(ta), "div component", Np, &path)) return rc;
    bool launched = false;
    if (path == kPathMfma)
        if (int rc = launch_nd2_np<1>(J, D, P, 1, E, Np, opT, s, &launched, jes)) return rc;
    if (!launched) {   // no MFMA geometry, or fewer elements than one wave tile
        if (!tiled_fits(ta)) return fail(FE_EUNSUPPORTED, "div component: no kernel for ndim = 2, Np = %d", Np);
        if (int rc = launch_tiled(ta, s)) return rc;
    }
    FE_HIP_CHECK(hipGetLastError());
    return FE_OK;
}

int fe_divcomp3d_f64(const double* J, const double* D, const double* u, double* out, int64_t E,
                     int32_t Np, int32_t op_flags, int32_t variant, void* stream) {
    forget_last_launch();
    if (int rc = check_common("div component", J, D, u, out, E, Np)) return rc;
    if (op_flags & ~(FE_OP_TRANSPOSED | FE_OP_J_ES))
        return fail(FE_EINVAL, "div component: bad operator flags %d", op_flags);
    if (variant < FE_VARIANT_AUTO || variant > FE_VARIANT_TILED)
        return fail(FE_EUNSUPPORTED, "div component: unknown variant %d", variant);
    if (E == 0) return FE_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int opT = (op_flags & FE_OP_TRANSPOSED) ? 1 : 0, jes = (op_flags & FE_OP_J_ES) ? 1 : 0;
    const bool mfma_ok = Np == 56 || Np == 35 || Np == 20 || Np == 10 || Np == 4;
    fe::FieldPtrs Pt = {};
    Pt.v[0] = u;
    Pt.out[0] = out;
    const fe::TiledArgs ta = tiled_args(FE_FAMILY_DIVCOMP, J, D, Pt, 1, E, 3, Np, 0, 0, opT, jes, 0);
    KernelPath path;
    if (int rc = choose_path(variant, mfma_ok, tiled_fits(ta), "div component", Np, &path)) return rc;
    if (path == kPathTiled) return launch_tiled(ta, s);
    int64_t e_done = 0;
    if (path == kPathMfma) {
        int rc = FE_OK;
        switch (Np) {   // wave tile = 16 M elements
            case 56: rc = launch_divcomp<56, 1, true>(J, D, u, out, E, opT, jes, s, &e_done); break;   // p = 5: A in LDS
            case 35: rc = launch_divcomp<35, 1>(J, D, u, out, E, opT, jes, s, &e_done); break;
            case 20: rc = launch_divcomp<20, 2>(J, D, u, out, E, opT, jes, s, &e_done); break;
            case 10: rc = launch_divcomp<10, 4>(J, D, u, out, E, opT, jes, s, &e_done); break;
            default: rc = launch_divcomp<4, 6>(J, D, u, out, E, opT, jes, s, &e_done); break;
        }
        if (rc != FE_OK) return rc;
    }
    if (e_done < E)
        hipLaunchKernelGGL(fe::divcomp3d_generic_kernel, dim3(generic_grid(E - e_done, Np)), dim3(256), 0, s,
                           J, D, u, out, E, Np, e_done, opT, jes);
    FE_HIP_CHECK(hipGetLastError());
    return FE_OK;
}

int fe_matapply_f64(const double* J, const double* D, const double* const* u, double* const* out, int64_t E,
                    int32_t Np, int32_t b, int32_t op_flags, int32_t variant, void* stream) {
    forget_last_launch();
    if (!u || !out) return fail(FE_EINVAL, "matapply: null pointer table");
    if (b < 1) return fail(FE_EINVAL, "matapply: b=%d, need at least one field", b);
    if (b > FE_MAX_FIELDS)   // FE_MAX_FIELDS fields per launch
        return fe::for_each_field_group(b, FE_MAX_FIELDS, false, [&](int k0, int nb) {
            return fe_matapply_f64(J, D, u + k0, out + k0, E, Np, nb, op_flags, variant, stream);
        });
    fe::FieldPtrs P = {};
    for (int k = 0; k < b; ++k) {
        if (int rc = check_common("matapply", J ? J : D, D, u[k], out[k], E, Np)) return rc;   // J is optional
        P.v[k] = u[k];
        P.out[k] = out[k];
    }
    if (op_flags & ~FE_OP_TRANSPOSED) return fail(FE_EINVAL, "matapply: bad operator flags %d", op_flags);
    if (variant < FE_VARIANT_AUTO || variant > FE_VARIANT_TILED)
        return fail(FE_EUNSUPPORTED, "matapply: unknown variant %d", variant);
    if (E == 0) return FE_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int opT = (op_flags & FE_OP_TRANSPOSED) ? 1 : 0;
    const bool mfma_ok = Np == 56 || Np == 35 || Np == 20 || Np == 15 || Np == 10 || Np == 6 || Np == 4 || Np == 3;
    const fe::TiledArgs ta = tiled_args(FE_FAMILY_MATAPPLY, J, D, P, b, E, 1, Np, 0, 0, opT, 0, 0);
    KernelPath path;
    if (int rc = choose_path(variant, mfma_ok, tiled_fits(ta), "matapply", Np, &path)) return rc;
    if (path == kPathTiled) return launch_tiled(ta, s);
    int64_t e_done = 0;
    if (path == kPathMfma) {
        int rc = FE_OK;
        switch (Np) {   // wave tile = 16 M elements: a few KB per tile at every order
            case 56: rc = launch_matapply<56, 1>(J, D, P, b, E, opT, s, &e_done); break;   // p = 5
            case 35: rc = launch_matapply<35, 2>(J, D, P, b, E, opT, s, &e_done); break;
            case 20: rc = launch_matapply<20, 4>(J, D, P, b, E, opT, s, &e_done); break;
            case 15: rc = launch_matapply<15, 4>(J, D, P, b, E, opT, s, &e_done); break;
            case 10: rc = launch_matapply<10, 6>(J, D, P, b, E, opT, s, &e_done); break;
            case 6: rc = launch_matapply<6, 8>(J, D, P, b, E, opT, s, &e_done); break;
            case 4: rc = launch_matapply<4, 8>(J, D, P, b, E, opT, s, &e_done); break;
            default: rc = launch_matapply<3, 8>(J, D, P, b, E, opT, s, &e_done); break;
        }
        if (rc != FE_OK) return rc;
    }
    if (e_done < E)
        for (int k = 0; k < b; ++k)
            hipLaunchKernelGGL(fe::matapply_generic_kernel, dim3(generic_grid(E - e_done, Np)), dim3(256), 0, s,
                               J, D, P.v[k], P.out[k], E, Np, e_done, opT);
    FE_HIP_CHECK(hipGetLastError());
    return FE_OK;
}

int fe_graddiv3d_f64(const double* J, const double* D, const double* u_grad, const double* v_div,
                     double* grad_out, double* div_out, int64_t E, int32_t Np, int32_t variant,
                     void* stream) {
    return fe_graddiv3d_prepared_f64(J, D, nullptr, u_grad, v_div, grad_out, div_out, E, Np, variant, stream);
}

int fe_graddiv3d_prepared_f64(const double* J, const double* D, const void* D_prepared, const double* u_grad,
                              const double* v_div, double* grad_out, double* div_out, int64_t E, int32_t Np,
                              int32_t variant, void* stream) {
    forget_last_launch();
    int perr;
    const void* prep = usable_prepared(D_prepared, D, kPreparedD, Np, 0, 0, 0, "graddiv", &perr);
    if (perr != FE_OK) return perr;
    if (int rc = check_common("graddiv", J, D, u_grad, grad_out, E, Np)) return rc;
    if (int rc = check_common("graddiv", J, D, v_div, div_out, E, Np)) return rc;
    if (variant < FE_VARIANT_AUTO || variant > FE_VARIANT_TILED)
        return fail(FE_EUNSUPPORTED, "graddiv: unknown variant %d", variant);
    if ((variant != FE_VARIANT_AUTO && variant != FE_VARIANT_MFMA) || !fe::is_tet_order(Np)) {
        // two launches back to back on the stream
        if (int rc = fe_div3d_prepared_f64(J, D, D_prepared, &v_div, &div_out, E, Np, 1, 0, variant, stream)) return rc;
        return fe_grad3d_prepared_f64(J, D, D_prepared, &u_grad, &grad_out, E, Np, 1, 0, variant, stream);
    }
    if (E == 0) return FE_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const fe::GradFields Pg = grad_fields(J, &u_grad, &grad_out, 1, E, Np);
    fe::FieldPtrs Pd = {};
    Pd.v[0] = v_div;  Pd.out[0] = div_out;
    int64_t done_g = 0, done_d = 0;
    if (int rc = fe::with_tet_order(Np, [&](auto o) {
            using O = decltype(o);
            return launch_graddiv<O::NP, O::MG, O::MD>(J, D, prep, Pg, Pd, E, s, &done_g, &done_d);
        }))
        return rc;
    if (done_d < E)
        hipLaunchKernelGGL(fe::div3d_generic_kernel, dim3(generic_grid(E - done_d, Np)), dim3(256), 0, s,
                           J, D, v_div, div_out, E, Np, done_d, 0);
    if (done_g < E)
        hipLaunchKernelGGL(fe::grad3d_generic_kernel, dim3(generic_grid(E - done_g, Np)), dim3(256), 0, s,
                           J, D, u_grad, grad_out, E, Np, done_g, 0);
    FE_HIP_CHECK(hipGetLastError());
    return FE_OK;
}

int fe_facemass_f64(const double* J, const double* R, const double* const* v, double* const* out,
                    int64_t E, int32_t Np, int32_t nf, int32_t Nfp, int32_t b,
                    int32_t layout_flags, int32_t variant, void* stream) {
    return fe_facemass_prepared_f64(J, R, nullptr, v, out, E, Np, nf, Nfp, b, layout_flags, variant, stream);
}

int fe_facemass_prepared_f64(const double* J, const double* R, const void* R_prepared, const double* const* v,
                             double* const* out, int64_t E, int32_t Np, int32_t nf, int32_t Nfp, int32_t b,
                             int32_t layout_flags, int32_t variant, void* stream) {
    forget_last_launch();
    int perr;   // (the J layout flag is not part of the operator)
    const void* prep = usable_prepared(R_prepared, R, kPreparedR, Np, nf, Nfp, layout_flags & ~FE_FM_J_FE, "face-mass", &perr);
    if (perr != FE_OK) return perr;
    CallCheck c = {"face-mass", J, R, ptr_table(v), ptr_table(out), E, Np, b, layout_flags, 7};
    c.flag_name = "layout";
    c.faces = true; c.nf = nf; c.Nfp = Nfp;
    c.variant = variant; c.variant_hi = FE_VARIANT_TILED;
    FE_CHECK_CALL(c);
    hipStream_t s = static_cast<hipStream_t>(stream);

    FmChoice geo{0, 16};
    const bool mfma_ok = fm_mfma_geometry(Np, nf, Nfp, &geo);
    const fe::FmLayout L(layout_flags, Np, nf, Nfp, E);
    const int jfe = L.jfe, rifj = L.rifj;
    KernelPath path;
    {
        fe::FieldPtrs none = {};
        const fe::TiledArgs probe = tiled_args(FE_FAMILY_FACEMASS, J, R, none, 1, E, 3, Np, nf, Nfp, 0, jfe, rifj);
        // below ~10 rows the tiled kernel has too few busy lanes to beat the plain one (measured:
        // triangles p = 2, Np = 6: 1.4 vs 2.2 TFLOP/s; p = 4, Np = 15: 3.1 vs 2.6)
        const bool tiled_ok = tiled_fits(probe) && (variant == FE_VARIANT_TILED || Np >= 10);
        if (int rc = choose_path(variant, mfma_ok, tiled_ok,
                                 "face-mass (MFMA: tetrahedra p = 1..5 or triangles p = 1..5)", Np, &path))
            return rc;
    }
    if (path == kPathTiled)   // groups of up to kMaxFields fields share the staged operator
        return fe::for_each_field_group(b, fe::kMaxFields, false, [&](int k0, int nb) {
            fe::FieldPtrs P = {};
            for (int k = 0; k < nb; ++k) { P.v[k] = v[k0 + k]; P.out[k] = out[k0 + k]; }
            return launch_tiled(tiled_args(FE_FAMILY_FACEMASS, J, R, P, nb, E, 3, Np, nf, Nfp, 0, jfe, rifj), s);
        });
    const bool use_mfma = path == kPathMfma;
    const int64_t nTiles = use_mfma ? E / geo.tel : 0;      // full wave tiles
    const int64_t e_done = nTiles > 0 ? E : 0;   // an MFMA launch covers the remainder too
    // fields go in groups of up to max_group per launch; two or more fields never leave a group of 1 for the MFMA kernel
    if (int rc = fe::for_each_field_group(b, use_mfma ? geo.max_group : fe::kMaxFields, use_mfma, [&](int k0, int nb) {
            const fe::FieldPtrs P = field_group(v + k0, out + k0, nb);
            if (nTiles > 0) {
                int rc = FE_OK;
                if (nf == 3) {
                    switch (Np) {   // triangles; wave tile = 16 M elements
                        case 21: rc = launch_fm<21, 6, 3, 3>(J, R, prep, P, nb, E, nTiles, jfe, rifj, s); break;
                        case 15: rc = launch_fm<15, 5, 4, 3>(J, R, prep, P, nb, E, nTiles, jfe, rifj, s); break;
                        case 10: rc = launch_fm<10, 4, 5, 3>(J, R, prep, P, nb, E, nTiles, jfe, rifj, s); break;
                        case 6: rc = launch_fm<6, 3, 6, 3>(J, R, prep, P, nb, E, nTiles, jfe, rifj, s); break;
                        default: rc = launch_fm<3, 2, 8, 3>(J, R, prep, P, nb, E, nTiles, jfe, rifj, s); break;
                    }
                } else if (Np == 56) {   // p = 5: A fragments in LDS
                    rc = launch_fm<56, 21, 1, fe::kFmNf, true>(J, R, prep, P, nb, E, nTiles, jfe, rifj, s);
                } else {
                    rc = fe::with_tet_order(Np, [&](auto o) {
                        using O = decltype(o);
                        return launch_fm<O::NP, O::NFP, O::MF>(J, R, prep, P, nb, E, nTiles, jfe, rifj, s);
                    });
                }
                if (rc != FE_OK) return rc;
            }
            if (e_done < E) {
                const dim3 grid(generic_grid(E - e_done, Np)), block(256);
                int launched = FE_OK;
                if (!fe::with_field_count<1, fe::kMaxFields>(nb, &launched, [&](auto NB) {
                        hipLaunchKernelGGL(fe::facemass_generic_kernel<decltype(NB)::value>, grid, block, 0, s, J, R, P, E, Np, nf, Nfp,
                                           L.jEs, L.jFs, L.rF, L.rI, L.rJ, e_done);
                        return FE_OK;
                    }))
                    return fail(FE_EINVAL, "face-mass: internal field grouping error (nb=%d)", nb);
            }
            return FE_OK;
        }))
        return rc;
    FE_HIP_CHECK(hipGetLastError());
    return FE_OK;
}

int fe_facemass_acc_f64(const double* J, const double* R, const double* const* v, double* const* out, int64_t E, int32_t Np,
                        int32_t nf, int32_t Nfp, int32_t b, int32_t layout_flags, double alpha, double beta, void* stream) {
    forget_last_launch();
    // the compiled scope: tetrahedra p = 1..4, two or more fields (in groups of 2..4); the caller evaluates anything else into
    // an array of its own and combines with fe_axpby
    CallCheck c = {"accumulating face-mass", J, R, ptr_table(v), ptr_table(out), E, Np, b, layout_flags, 7};
    c.flag_name = "layout";
    c.alpha = &alpha; c.beta = &beta;
    c.faces = true; c.nf = nf; c.Nfp = Nfp;
    c.scope = kScopeTetFaces; c.min_b = 2; c.kernel = "fused kernel";
    FE_CHECK_CALL(c);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const fe::FmLayout L(layout_flags, Np, nf, Nfp, E);
    // fields go in groups of up to four per launch; never leave a group of one
    if (int rc = fe::for_each_field_group(b, 4, true, [&](int k0, int nb) {
            const fe::FieldPtrs P = field_group(v + k0, out + k0, nb);
            return fe::with_tet_order(Np, [&](auto o) {
                using O = decltype(o);
                // full wave tiles; the launch covers the elements behind the last one too
                if (const int64_t nTiles = E / (16 * O::MF))
                    return launch_fm_acc<O::NP, O::NFP, O::MF>(J, R, P, nb, E, nTiles, L.jfe, L.rifj, alpha, beta, s);
                int rc = FE_OK;   // fewer elements than a wave tile: one thread per entry
                if (!fe::with_field_count<2, 4>(nb, &rc, [&](auto NB) {
                        hipLaunchKernelGGL(fe::facemass_generic_acc_kernel<decltype(NB)::value>, dim3(generic_grid(E, Np)), dim3(256), 0, s,
                                           J, R, P, E, Np, nf, Nfp, L.jEs, L.jFs, L.rF, L.rI, L.rJ, (int64_t)0, alpha, beta);
                        return FE_OK;
                    }))
                    return fail(FE_EINVAL, "accumulating face-mass: internal field grouping error (nb=%d)", nb);
                return rc;
            });
        }))
        return rc;
    FE_HIP_CHECK(hipGetLastError());
    return FE_OK;
}

int fe_grad3d_acc_f64(const double* J, const double* D, const double* u, double* out, int64_t E, int32_t Np, int32_t op_flags,
                      double alpha, double beta, void* stream) {
    forget_last_launch();
    // the compiled scope: tetrahedra p = 1..4; the caller evaluates anything else into an array of its own and combines with fe_axpby
    CallCheck c = {"accumulating grad", J, D, ptr_table(&u), ptr_table(&out), E, Np, 1, op_flags, FE_OP_TRANSPOSED};
    c.alpha = &alpha; c.beta = &beta;
    c.scope = kScopeTet; c.kernel = "accumulating kernel";
    FE_CHECK_CALL(c);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int opT = (op_flags & FE_OP_TRANSPOSED) ? 1 : 0;
    const fe::GradFields P = grad_fields(J, &u, &out, 1, E, Np);
    bool launched = false;
    if (int rc = fe::with_tet_order(Np, [&](auto o) {
            using O = decltype(o);
            return launch_grad_acc<O::NP, O::MG>(P, D, E, opT, alpha, beta, s, &launched);
        }))
        return rc;
    if (!launched) {   // fewer elements than a wave tile: one thread per entry
        hipLaunchKernelGGL(fe::grad3d_generic_acc_kernel, dim3(generic_grid(E, Np)), dim3(256), 0, s, J, D, u, out, E, Np,
                           (int64_t)0, opT, alpha, beta);
    }
    FE_HIP_CHECK(hipGetLastError());
    return FE_OK;
}

int fe_div3d_acc_f64(const double* J, const double* D, const double* u, double* out, int64_t E, int32_t Np, int32_t op_flags,
                     double alpha, double beta, void* stream) {
    forget_last_launch();
    CallCheck c = {"accumulating div", J, D, ptr_table(&u), ptr_table(&out), E, Np, 1, op_flags, FE_OP_TRANSPOSED};
    c.alpha = &alpha; c.beta = &beta;
    c.scope = kScopeTet; c.kernel = "accumulating kernel";
    FE_CHECK_CALL(c);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int opT = (op_flags & FE_OP_TRANSPOSED) ? 1 : 0;
    fe::FieldPtrs P = {};
    P.v[0] = u;
    P.out[0] = out;
    bool launched = false;
    if (int rc = fe::with_tet_order(Np, [&](auto o) {
            using O = decltype(o);
            return launch_div_acc<O::NP, O::MD>(J, D, P, E, opT, alpha, beta, s, &launched);
        }))
        return rc;
    if (!launched) {
        hipLaunchKernelGGL(fe::div3d_generic_acc_kernel, dim3(generic_grid(E, Np)), dim3(256), 0, s, J, D, u, out, E, Np,
                           (int64_t)0, opT, alpha, beta);
    }
    FE_HIP_CHECK(hipGetLastError());
    return FE_OK;
}

// ---- element slices of larger arrays: E elements, plane distances (leading dimensions) of their own.
int fe_grad3d_strided_f64(const double* J, int64_t ldJ, const double* D, const double* const* u, double* const* out, int64_t ldOut,
                          int64_t E, int32_t Np, int32_t b, int32_t op_flags, void* stream) {
    forget_last_launch();
    CallCheck c = {"grad on an element slice", J, D, ptr_table(u), ptr_table(out), E, Np, b, op_flags, FE_OP_TRANSPOSED};
    use_ld(c, 0, ldJ);
    use_ld(c, 2, ldOut);
    c.scope = kScopeTet; c.scope_first = true;
    FE_CHECK_CALL(c);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int opT = (op_flags & FE_OP_TRANSPOSED) ? 1 : 0;
    if (int rc = fe::for_each_field_group(b, fe::kMaxFields, false, [&](int k0, int nb) {   // kMaxFields fields per launch
            fe::GradFields P = {};
            for (int x = 0; x < 3; ++x) P.j[x] = J + (int64_t)x * 3 * ldJ;
            for (int k = 0; k < nb; ++k) {
                P.u[k] = u[k0 + k];
                for (int x = 0; x < 3; ++x) P.out[k][x] = out[k0 + k] + (int64_t)x * ldOut * Np;
            }
            bool launched = false;
            if (int rc = fe::with_tet_order(Np, [&](auto o) {
                    using O = decltype(o);
                    return launch_grad_strided<O::NP, O::MG>(P, D, nb, E, ldJ, ldOut, opT, s, &launched);
                }))
                return rc;
            if (!launched)   // fewer elements than a wave tile: one thread per entry
                for (int k = 0; k < nb; ++k)
                    hipLaunchKernelGGL(fe::grad3d_generic_ld_kernel, dim3(generic_grid(E, Np)), dim3(256), 0, s, J, D, P.u[k], P.out[k][0],
                                       E, ldJ, ldOut, Np, opT);
            return FE_OK;
        }))
        return rc;
    FE_HIP_CHECK(hipGetLastError());
    return FE_OK;
}

int fe_div3d_strided_f64(const double* J, int64_t ldJ, const double* D, const double* const* u, int64_t ldIn, double* const* out,
                         int64_t E, int32_t Np, int32_t b, int32_t op_flags, void* stream) {
    forget_last_launch();
    CallCheck c = {"div on an element slice", J, D, ptr_table(u), ptr_table(out), E, Np, b, op_flags, FE_OP_TRANSPOSED};
    use_ld(c, 0, ldJ);
    use_ld(c, 1, ldIn);
    c.scope = kScopeTet; c.scope_first = true;
    FE_CHECK_CALL(c);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int opT = (op_flags & FE_OP_TRANSPOSED) ? 1 : 0;
    if (int rc = fe::for_each_field_group(b, fe::kMaxFields, false, [&](int k0, int nb) {   // kMaxFields fields per launch
            const fe::FieldPtrs P = field_group(u + k0, out + k0, nb);
            bool launched = false;
            if (int rc = fe::with_tet_order(Np, [&](auto o) {
                    using O = decltype(o);
                    return launch_div_strided<O::NP, O::MD>(J, D, P, nb, E, ldJ, ldIn, opT, s, &launched);
                }))
                return rc;
            if (!launched)
                for (int k = 0; k < nb; ++k)
                    hipLaunchKernelGGL(fe::div3d_generic_ld_kernel, dim3(generic_grid(E, Np)), dim3(256), 0, s, J, D, P.v[k], P.out[k], E,
                                       ldJ, ldIn, Np, opT);
            return FE_OK;
        }))
        return rc;
    FE_HIP_CHECK(hipGetLastError());
    return FE_OK;
}

int fe_facemass_strided_f64(const double* J, int64_t ldJ, const double* R, const double* const* v, int64_t ldIn, double* const* out,
                            int64_t E, int32_t Np, int32_t nf, int32_t Nfp, int32_t b, int32_t layout_flags, void* stream) {
    forget_last_launch();
    // the compiled scope: tetrahedra p = 1..4, two or more fields (in groups of 2..4)
    CallCheck c = {"face-mass on an element slice", J, R, ptr_table(v), ptr_table(out), E, Np, b, layout_flags, 7};
    c.flag_name = "layout";
    if (layout_flags & FE_FM_J_FE) use_ld(c, 0, ldJ);   // (J[E][nf] has no plane distance)
    use_ld(c, 1, ldIn);
    c.faces = true; c.nf = nf; c.Nfp = Nfp;
    c.scope = kScopeTetFaces; c.min_b = 2; c.scope_first = true;
    FE_CHECK_CALL(c);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const fe::FmLayout L(layout_flags, Np, nf, Nfp, ldJ);
    // fields go in groups of up to four per launch; never leave a group of one
    if (int rc = fe::for_each_field_group(b, 4, true, [&](int k0, int nb) {
            const fe::FieldPtrs P = field_group(v + k0, out + k0, nb);
            return fe::with_tet_order(Np, [&](auto o) {
                using O = decltype(o);
                // full wave tiles; the launch covers the elements behind the last one too
                if (const int64_t nTiles = E / (16 * O::MF))
                    return launch_fm_strided<O::NP, O::NFP, O::MF>(J, R, P, nb, E, ldJ, ldIn, nTiles, L.jfe, L.rifj, s);
                int rc = FE_OK;   // fewer elements than a wave tile: one thread per entry
                if (!fe::with_field_count<2, 4>(nb, &rc, [&](auto NB) {
                        hipLaunchKernelGGL(fe::facemass_generic_ld_kernel<decltype(NB)::value>, dim3(generic_grid(E, Np)), dim3(256), 0, s,
                                           J, R, P, E, ldIn, Np, nf, Nfp, L.jEs, L.jFs, L.rF, L.rI, L.rJ);
                        return FE_OK;
                    }))
                    return fail(FE_EINVAL, "face-mass on an element slice: internal field grouping error (nb=%d)", nb);
                return rc;
            });
        }))
        return rc;
    FE_HIP_CHECK(hipGetLastError());
    return FE_OK;
}

// out <- alpha x + beta out over n contiguous entries (fe_einsum.h, axpby_kernel)
int fe_axpby(void* out, const void* x, int64_t n, double alpha, double beta, int32_t dtype, void* stream) {
    if (n < 0) return fail(FE_EINVAL, "axpby: n must be >= 0 (got %lld)", (long long)n);
    if (dtype != FE_DTYPE_F64 && dtype != FE_DTYPE_F32) return fail(FE_EINVAL, "axpby: dtype %d is neither float64 nor float32", dtype);
    if (!std::isfinite(alpha) || !std::isfinite(beta)) return fail(FE_EINVAL, "axpby: alpha and beta must be finite (got %g, %g)", alpha, beta);
    if (n == 0) return FE_OK;
    if (!out || !x) return fail(FE_EINVAL, "axpby: null device pointer");
    const uintptr_t size = dtype == FE_DTYPE_F64 ? 8 : 4;
    if ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(x)) % size)
        return fail(FE_EINVAL, "axpby: pointers must be aligned to the element size (%d bytes)", (int)size);
    if (n >= ((int64_t)1 << 39)) return fail(FE_EINVAL, "axpby: n too large");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t per = 16 / (int64_t)size;
    const int64_t want = (n / per + 255) / 256 + 1, cap = 32 * (int64_t)device_cu_count();
    const dim3 grid((unsigned)(want < cap ? want : cap)), block(256);
    if (dtype == FE_DTYPE_F64)
        hipLaunchKernelGGL(fe::axpby_kernel<double>, grid, block, 0, s, static_cast<double*>(out), static_cast<const double*>(x), n,
                           alpha, beta);
    else
        hipLaunchKernelGGL(fe::axpby_kernel<float>, grid, block, 0, s, static_cast<float*>(out), static_cast<const float*>(x), n,
                           (float)alpha, (float)beta);
    FE_HIP_CHECK(hipGetLastError());
    return FE_OK;
}

int fe_waveop3d_f64(const double* J, const double* D, const double* u_grad, double* grad_out,
                    const double* v_div, double* div_out, const double* Jface, const double* R,
                    const double* const* f, double* const* lift, int64_t E, int32_t Np, int32_t nf,
                    int32_t Nfp, int32_t b, int32_t fm_layout_flags, int32_t variant, void* stream) {
    return fe_waveop3d_prepared_f64(J, D, nullptr, u_grad, grad_out, v_div, div_out, Jface, R, nullptr, f, lift, E, Np, nf,
                                    Nfp, b, fm_layout_flags, variant, stream);
}

int fe_waveop3d_prepared_f64(const double* J, const double* D, const void* D_prepared, const double* u_grad,
                             double* grad_out, const double* v_div, double* div_out, const double* Jface,
                             const double* R, const void* R_prepared, const double* const* f, double* const* lift,
                             int64_t E, int32_t Np, int32_t nf, int32_t Nfp, int32_t b, int32_t fm_layout_flags,
                             int32_t variant, void* stream) {
    forget_last_launch();
    int perr;
    const void* prepD = usable_prepared(D_prepared, D, kPreparedD, Np, 0, 0, 0, "waveop", &perr);
    if (perr != FE_OK) return perr;
    const void* prepR = usable_prepared(R_prepared, R, kPreparedR, Np, nf, Nfp, fm_layout_flags & ~FE_FM_J_FE, "waveop", &perr);
    if (perr != FE_OK) return perr;
    FmChoice geo{0, 16};
    const bool fused = (variant == FE_VARIANT_AUTO || variant == FE_VARIANT_MFMA) && nf == fe::kFmNf && Np != 56 &&
                       fm_mfma_geometry(Np, nf, Nfp, &geo) && b >= 2 &&
                       b <= 4 && f && lift && E > 0 && !(fm_layout_flags & ~7);
    if (!fused) {   // three launches (argument checks included)
        if (int rc = fe_graddiv3d_prepared_f64(J, D, D_prepared, u_grad, v_div, grad_out, div_out, E, Np, variant, stream))
            return rc;
        return fe_facemass_prepared_f64(Jface, R, R_prepared, f, lift, E, Np, nf, Nfp, b, fm_layout_flags, variant, stream);
    }
    if (int rc = check_common("waveop", J, D, u_grad, grad_out, E, Np)) return rc;
    if (int rc = check_common("waveop", J, D, v_div, div_out, E, Np)) return rc;
    if (variant < FE_VARIANT_AUTO || variant > FE_VARIANT_TILED)
        return fail(FE_EUNSUPPORTED, "waveop: unknown variant %d", variant);
    if (!Jface || !R) return fail(FE_EINVAL, "waveop: null device pointer");
    uintptr_t bits = reinterpret_cast<uintptr_t>(Jface) | reinterpret_cast<uintptr_t>(R);
    for (int k = 0; k < b; ++k) {
        if (!f[k] || !lift[k]) return fail(FE_EINVAL, "waveop: null field pointer %d", k);
        bits |= reinterpret_cast<uintptr_t>(f[k]) | reinterpret_cast<uintptr_t>(lift[k]);
    }
    if (bits & 7u) return fail(FE_EINVAL, "waveop: device pointers must be 8-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const fe::GradFields Pg = grad_fields(J, &u_grad, &grad_out, 1, E, Np);
    fe::FieldPtrs Pd = {};
    Pd.v[0] = v_div;  Pd.out[0] = div_out;
    const fe::FieldPtrs Pf = field_group(f, lift, b);
    fe::WaveOpArgs a = {};
    a.J = J; a.D = D; a.Jf = Jface; a.R = R; a.E = E;
    a.prepD = prepD; a.prepR = prepR;
    const fe::FmLayout L(fm_layout_flags, Np, nf, Nfp, E);
    a.jfe = L.jfe;
    a.rlayout = L.rifj;
    bool launched = false;
    if (int rc = fe::with_tet_order(Np, [&](auto o) {
            using O = decltype(o);
            return launch_waveop<O::NP, O::NFP, O::MG, O::MD, O::MF>(a, Pg, Pd, Pf, b, s, &launched);
        }))
        return rc;
    if (!launched) {   // fewer elements than any wave tile: the generic kernels
        if (int rc2 = fe_graddiv3d_f64(J, D, u_grad, v_div, grad_out, div_out, E, Np, variant, stream)) return rc2;
        return fe_facemass_f64(Jface, R, f, lift, E, Np, nf, Nfp, b, fm_layout_flags, variant, stream);
    }
    (void)prepD; (void)prepR;
    FE_HIP_CHECK(hipGetLastError());
    return FE_OK;
}

int fe_einsum_generic(const fe_einsum_desc* d, const void* const* operands, void* out,
                      void* stream) {
    if (!d || !operands) return fail(FE_EINVAL, "einsum: null descriptor");
    if (d->n_operands < 1 || d->n_operands > FE_MAX_EINSUM_OPERANDS || d->n_out < 0 ||
        d->n_out > FE_MAX_EINSUM_INDICES || d->n_sum < 0 || d->n_sum > FE_MAX_EINSUM_INDICES)
        return fail(FE_EINVAL, "einsum: %d operands / %d output / %d summation indices out of range",
                    d->n_operands, d->n_out, d->n_sum);
    unsigned f32_mask = 0;
    if (int rc = einsum_dtype("einsum", d, &f32_mask)) return rc;
    int64_t n_out = 1, n_sum = 1;
    for (int k = 0; k < d->n_out; ++k) {
        if (d->out_extent[k] < 0) return fail(FE_EINVAL, "einsum: negative extent");
        n_out *= d->out_extent[k];
    }
    for (int k = 0; k < d->n_sum; ++k) {
        if (d->sum_extent[k] < 0) return fail(FE_EINVAL, "einsum: negative extent");
        n_sum *= d->sum_extent[k];
    }
    if (n_out == 0) return FE_OK;
    if (!out) return fail(FE_EINVAL, "einsum: null output pointer");
    if (n_out >= ((int64_t)1 << 39)) return fail(FE_EINVAL, "einsum: output too large");
    fe_einsum_ptrs P;
    for (int p = 0; p < FE_MAX_EINSUM_OPERANDS; ++p) P.p[p] = nullptr;
    for (int p = 0; p < d->n_operands; ++p) {
        if (!operands[p] && n_sum > 0) return fail(FE_EINVAL, "einsum: null operand %d", p);
        P.p[p] = operands[p];
        if (f32_mask && reinterpret_cast<uintptr_t>(operands[p]) % ((f32_mask >> p & 1) ? 4 : 8))
            return fail(FE_EINVAL, "einsum: operand %d not aligned to its element size", p);
    }
    if (f32_mask && reinterpret_cast<uintptr_t>(out) % 8) return fail(FE_EINVAL, "einsum: output not 8-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 block(256);
    const bool f64 = d->dtype == FE_DTYPE_F64 || f32_mask;
    if (d->n_sum > 0 && n_sum == 0) {   // a summation index of extent 0: every output entry is an empty sum
        FE_HIP_CHECK(hipMemsetAsync(out, 0, (size_t)n_out * (f64 ? 8 : 4), s));
        return FE_OK;
    }

    // pointwise product of congruent contiguous operands: a vectorised stream
    bool pointwise = d->n_sum == 0;
    for (int p = 0; p < d->n_operands && pointwise; ++p) {
        int64_t dense = 1;
        for (int k = d->n_out - 1; k >= 0; --k) {
            if (d->out_extent[k] != 1 && d->op_out_stride[p][k] != dense) pointwise = false;
            dense *= d->out_extent[k];
        }
    }
    if (pointwise) {
        const int64_t want = (n_out / 2 + 255) / 256 + 1, cap = 32 * (int64_t)device_cu_count();
        const dim3 grid((unsigned)(want < cap ? want : cap));
        if (f32_mask)
            hipLaunchKernelGGL(fe::einsum_pointwise_mixed_kernel, grid, block, 0, s, P, d->n_operands, f32_mask,
                               static_cast<double*>(out), n_out);
        else if (f64)
            hipLaunchKernelGGL(fe::einsum_pointwise_kernel<double>, grid, block, 0, s, P, d->n_operands,
                               static_cast<double*>(out), n_out);
        else
            hipLaunchKernelGGL(fe::einsum_pointwise_kernel<float>, grid, block, 0, s, P, d->n_operands,
                               static_cast<float*>(out), n_out);
        FE_HIP_CHECK(hipGetLastError());
        return FE_OK;
    }

    // lanes per output entry: > 1 when the fastest summation index is contiguous in an operand
    int group = 1;
    if (d->n_sum > 0 && n_sum >= 8) {
        bool contiguous = false;
        for (int p = 0; p < d->n_operands; ++p) contiguous |= d->op_sum_stride[p][d->n_sum - 1] == 1;
        if (contiguous) group = n_sum >= 32 ? 16 : 4;
    }
    if (n_out * group >= ((int64_t)1 << 39)) group = 1;
    const dim3 grid((unsigned)((n_out * group + 255) / 256));
#define FE_EINSUM_CASE(T, G) \
    hipLaunchKernelGGL((fe::einsum_generic_kernel<T, G>), grid, block, 0, s, *d, P, static_cast<T*>(out), n_out, n_sum)
#define FE_EINSUM_MIXED_CASE(G)                                                                                 \
    hipLaunchKernelGGL((fe::einsum_generic_kernel<double, G, true>), grid, block, 0, s, *d, P, static_cast<double*>(out), n_out, \
                       n_sum)
    if (f32_mask) {
        if (group == 16) FE_EINSUM_MIXED_CASE(16);
        else if (group == 4) FE_EINSUM_MIXED_CASE(4);
        else FE_EINSUM_MIXED_CASE(1);
    } else if (f64) {
        if (group == 16) FE_EINSUM_CASE(double, 16);
        else if (group == 4) FE_EINSUM_CASE(double, 4);
        else FE_EINSUM_CASE(double, 1);
    } else {
        if (group == 16) FE_EINSUM_CASE(float, 16);
        else if (group == 4) FE_EINSUM_CASE(float, 4);
        else FE_EINSUM_CASE(float, 1);
    }
#undef FE_EINSUM_CASE
#undef FE_EINSUM_MIXED_CASE
    FE_HIP_CHECK(hipGetLastError());
    return FE_OK;
}

// fe_einsum_contract, and (split: not null) the split-K launch of fe_einsum_reduce, which writes split->slices partial
// outputs into split->ws instead of `out`.  acc (not null, never with split): out <- alpha E + beta out in the store
// epilogue of the ACC instantiations (fe_einsum_contract_acc).
static int contract_launch(const fe_einsum_desc* d, const void* const* operands, void* out, void* stream,
                           const SplitK* split, const AccScale* acc = nullptr) {
    if (!d || !operands) return fail(FE_EINVAL, "contract: null descriptor");
    if (d->n_operands != 2)
        return fail(FE_EUNSUPPORTED, "contract: %d operands (the contraction kernel takes exactly 2)", d->n_operands);
    if (d->n_out < 0 || d->n_out > FE_MAX_EINSUM_INDICES || d->n_sum < 0 || d->n_sum > FE_MAX_EINSUM_INDICES)
        return fail(FE_EINVAL, "contract: %d output / %d summation indices out of range", d->n_out, d->n_sum);
    unsigned f32_mask = 0;
    if (int rc = einsum_dtype("contract", d, &f32_mask)) return rc;
    int64_t n_out = 1;
    for (int k = 0; k < d->n_out; ++k) {
        if (d->out_extent[k] < 0) return fail(FE_EINVAL, "contract: negative extent");
        n_out *= d->out_extent[k];
    }
    for (int k = 0; k < d->n_sum; ++k)
        if (d->sum_extent[k] < 0) return fail(FE_EINVAL, "contract: negative extent");
    if (n_out == 0) return FE_OK;
    if (!out) return fail(FE_EINVAL, "contract: null output pointer");
    if (n_out >= ((int64_t)1 << 39)) return fail(FE_EINVAL, "contract: output too large");
    const bool f64 = d->dtype == FE_DTYPE_F64 || f32_mask;
    const size_t esize = f64 ? 8 : 4;
    if (reinterpret_cast<uintptr_t>(out) % esize)
        return fail(FE_EINVAL, "contract: output pointer not aligned to its element size");

    // Group the indices (contract_groups); the output's innermost index of extent > 1 decides the orientation
    int32_t og[FE_MAX_EINSUM_INDICES], sg[FE_MAX_EINSUM_INDICES];
    contract_groups(d, og, sg);
    fe::ContractPlan P;
    memset(&P, 0, sizeof(P));
    int64_t sc = 1;
    char tail = 0;   // group of the output's innermost index of extent > 1: 'b', 'm' or 'n'
    int64_t oc[FE_MAX_EINSUM_INDICES];
    for (int k = d->n_out - 1; k >= 0; --k) {
        oc[k] = sc;
        sc *= d->out_extent[k];
    }
    for (int k = 0; k < d->n_out; ++k) {
        const int64_t e = d->out_extent[k], sa = d->op_out_stride[0][k], sb = d->op_out_stride[1][k];
        if (og[k] == FE_CONTRACT_BATCH) {
            P.b_ext[P.nb] = e, P.b_sa[P.nb] = sa, P.b_sb[P.nb] = sb, P.b_sc[P.nb] = oc[k], ++P.nb;
            tail = 'b';
        } else if (og[k] == FE_CONTRACT_M) {
            P.m_ext[P.nm] = e, P.m_sa[P.nm] = sa, P.m_sc[P.nm] = oc[k], ++P.nm;
            tail = 'm';
        } else if (og[k] == FE_CONTRACT_N) {
            P.n_ext[P.nn] = e, P.n_sb[P.nn] = sb, P.n_sc[P.nn] = oc[k], ++P.nn;
            tail = 'n';
        }
    }
    bool empty_k = false;
    int korder[FE_MAX_EINSUM_INDICES], nk = 0;
    for (int k = 0; k < d->n_sum; ++k) {
        if (d->sum_extent[k] == 0) empty_k = true;
        if (sg[k] == FE_CONTRACT_K) korder[nk++] = k;
    }
    // the output's contiguous index goes on the MFMA column (n): lanes store consecutive addresses
    const void* opA = operands[0];
    const void* opB = operands[1];
    int ia = 0, ib = 1;
    bool a_f32 = f32_mask & 1, b_f32 = f32_mask & 2;   // (mixed: which operand is stored as float32)
    if (tail == 'm') {
        std::swap(opA, opB);
        std::swap(a_f32, b_f32);
        std::swap(ia, ib);
        std::swap(P.nm, P.nn);
        for (int j = 0; j < FE_MAX_EINSUM_INDICES; ++j) {
            std::swap(P.m_ext[j], P.n_ext[j]);
            std::swap(P.m_sa[j], P.n_sb[j]);
            std::swap(P.m_sc[j], P.n_sc[j]);
            std::swap(P.b_sa[j], P.b_sb[j]);
        }
    }
    // summed indices: largest stride outermost, so that a unit-stride k index is the innermost one
    auto kkey = [&](int k) {
        const int64_t a = std::abs(d->op_sum_stride[ia][k]), b = std::abs(d->op_sum_stride[ib][k]);
        return a > b ? a : b;
    };
    for (int i = 1; i < nk; ++i)
        for (int j = i; j > 0 && kkey(korder[j - 1]) < kkey(korder[j]); --j) std::swap(korder[j - 1], korder[j]);
    P.nk = nk;
    P.K = empty_k ? 0 : 1;
    for (int j = 0; j < nk; ++j) {
        P.k_ext[j] = d->sum_extent[korder[j]];
        P.k_sa[j] = d->op_sum_stride[ia][korder[j]];
        P.k_sb[j] = d->op_sum_stride[ib][korder[j]];
        P.K *= P.k_ext[j];
    }
    if (P.K > 0 && (!opA || !opB)) return fail(FE_EINVAL, "contract: null operand");
    const size_t esizeA = a_f32 ? 4 : esize, esizeB = b_f32 ? 4 : esize;
    if (reinterpret_cast<uintptr_t>(opA) % esizeA || reinterpret_cast<uintptr_t>(opB) % esizeB)
        return fail(FE_EINVAL, "contract: operand pointer not aligned to its element size");
    P.M = P.N = 1;
    int64_t nbatch = 1;
    for (int j = 0; j < P.nm; ++j) P.M *= P.m_ext[j];
    for (int j = 0; j < P.nn; ++j) P.N *= P.n_ext[j];
    for (int j = 0; j < P.nb; ++j) nbatch *= P.b_ext[j];

    // fast direction of each operand: its rows when its innermost row index is contiguous and its innermost k is not
    const int mlast = P.nm - 1, nlast = P.nn - 1, klast = nk - 1;
    P.a_mfast = mlast >= 0 && P.m_sa[mlast] == 1 && !(klast >= 0 && P.k_sa[klast] == 1);
    P.b_mfast = nlast >= 0 && P.n_sb[nlast] == 1 && !(klast >= 0 && P.k_sb[klast] == 1);
    const int64_t fastA = P.a_mfast ? P.m_ext[mlast] : (klast >= 0 ? P.k_ext[klast] : 1);
    const int64_t fastB = P.b_mfast ? P.n_ext[nlast] : (klast >= 0 ? P.k_ext[klast] : 1);
    P.a_vstep = P.a_mfast ? P.m_sa[mlast] : (klast >= 0 ? P.k_sa[klast] : 0);
    P.b_vstep = P.b_mfast ? P.n_sb[nlast] : (klast >= 0 ? P.k_sb[klast] : 0);
    // 16-byte groups: one width for both operands of one dtype, each operand's own when they are mixed
    const int vmax = f64 ? 2 : 4, vmaxA = (int)(16 / esizeA), vmaxB = (int)(16 / esizeB);
    const int V = (fastA % vmax == 0 && fastB % vmax == 0) ? vmax : 1;
    int VA = f32_mask ? (fastA % vmaxA == 0 ? vmaxA : 1) : V;
    int VB = f32_mask ? (fastB % vmaxB == 0 ? vmaxB : 1) : V;
    if (a_f32 && b_f32) VA = VB = (VA > 1 && VB > 1) ? 4 : 1;   // (both float32 under float64: one width)
    // one vector load per group: unit stride inside it, a 16-byte aligned base, every other stride a multiple of V
    auto vec_ok = [&](const void* p, int V, size_t esize, bool mfast, int64_t vstep, const int64_t* sb_,
                      const int64_t* srow, int nrow, const int64_t* sk) {
        if (V == 1 || vstep != 1 || reinterpret_cast<uintptr_t>(p) % (V * esize)) return false;
        for (int j = 0; j < P.nb; ++j) if (sb_[j] % V) return false;
        for (int j = 0; j < nrow; ++j) if (srow[j] % V && !(mfast && j == nrow - 1)) return false;
        for (int j = 0; j < nk; ++j) if (sk[j] % V && !(!mfast && j == nk - 1)) return false;
        return true;
    };
    P.a_vec = vec_ok(opA, VA, esizeA, P.a_mfast, P.a_vstep, P.b_sa, P.m_sa, P.nm, P.k_sa);
    P.b_vec = vec_ok(opB, VB, esizeB, P.b_mfast, P.b_vstep, P.b_sb, P.n_sb, P.nn, P.k_sb);

    P.tiles_m = (P.M + fe::kCtBM - 1) / fe::kCtBM;
    P.tiles_n = (P.N + fe::kCtBM - 1) / fe::kCtBM;
    P.n_tiles = nbatch * P.tiles_m * P.tiles_n;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t cap = (int64_t)fe::kCtBlocksPerCu * device_cu_count();
    if (split) {
        P.k_slices = split->slices;
        P.k_slice_len = split->slice_len;
        P.c_size = n_out;
        const int64_t items = P.n_tiles * P.k_slices;
        const dim3 sgrid((unsigned)(items < cap ? items : cap)), sblock(fe::kCtThreads);
#define FE_CONTRACT_SPLIT_CASE(T, TA, TB, VVA, VVB, NAME)                                                               \
    do {                                                                                                                \
        static PerDeviceOnce once;                                                                                      \
        if (int rc = configured(once, fe::contract_mfma_kernel<T, VVA, TA, TB, VVB, true>, NAME, 0, fe::kCtThreads,     \
                                fe::kCtBlocksPerCu))                                                                    \
            return rc;                                                                                                  \
        hipLaunchKernelGGL((fe::contract_mfma_kernel<T, VVA, TA, TB, VVB, true>), sgrid, sblock, 0, s, P,               \
                           static_cast<const TA*>(opA), static_cast<const TB*>(opB), static_cast<T*>(split->ws));       \
    } while (0)
        if (a_f32 && b_f32) {
            if (VA > 1) FE_CONTRACT_SPLIT_CASE(double, float, float, 4, 4, "contract split-K f32 x f32 -> f64 (16-byte groups)");
            else FE_CONTRACT_SPLIT_CASE(double, float, float, 1, 1, "contract split-K f32 x f32 -> f64");
        } else if (a_f32) {
            if (VA > 1 && VB > 1) FE_CONTRACT_SPLIT_CASE(double, float, double, 4, 2, "contract split-K f32 x f64 (16-byte groups)");
            else if (VA > 1) FE_CONTRACT_SPLIT_CASE(double, float, double, 4, 1, "contract split-K f32 x f64 (A 16-byte groups)");
            else if (VB > 1) FE_CONTRACT_SPLIT_CASE(double, float, double, 1, 2, "contract split-K f32 x f64 (B 16-byte groups)");
            else FE_CONTRACT_SPLIT_CASE(double, float, double, 1, 1, "contract split-K f32 x f64");
        } else if (b_f32) {
            if (VA > 1 && VB > 1) FE_CONTRACT_SPLIT_CASE(double, double, float, 2, 4, "contract split-K f64 x f32 (16-byte groups)");
            else if (VA > 1) FE_CONTRACT_SPLIT_CASE(double, double, float, 2, 1, "contract split-K f64 x f32 (A 16-byte groups)");
            else if (VB > 1) FE_CONTRACT_SPLIT_CASE(double, double, float, 1, 4, "contract split-K f64 x f32 (B 16-byte groups)");
            else FE_CONTRACT_SPLIT_CASE(double, double, float, 1, 1, "contract split-K f64 x f32");
        } else if (f64) {
            if (V > 1) FE_CONTRACT_SPLIT_CASE(double, double, double, 2, 2, "contract split-K f64 (16-byte groups)");
            else FE_CONTRACT_SPLIT_CASE(double, double, double, 1, 1, "contract split-K f64");
        } else {
            if (V > 1) FE_CONTRACT_SPLIT_CASE(float, float, float, 4, 4, "contract split-K f32 (16-byte groups)");
            else FE_CONTRACT_SPLIT_CASE(float, float, float, 1, 1, "contract split-K f32");
        }
#undef FE_CONTRACT_SPLIT_CASE
        FE_HIP_CHECK(hipGetLastError());
        return FE_OK;
    }
    const dim3 grid((unsigned)(P.n_tiles < cap ? P.n_tiles : cap)), block(fe::kCtThreads);
    if (acc) {   // the ladder below, on the accumulating instantiations
#define FE_CONTRACT_ACC_CASE(T, TA, TB, VVA, VVB, NAME)                                                                 \
    do {                                                                                                                \
        static PerDeviceOnce once;                                                                                      \
        if (int rc = configured(once, fe::contract_mfma_kernel<T, VVA, TA, TB, VVB, false, true, T, T>, NAME " acc", 0, \
                                fe::kCtThreads, fe::kCtBlocksPerCu))                                                    \
            return rc;                                                                                                  \
        hipLaunchKernelGGL((fe::contract_mfma_kernel<T, VVA, TA, TB, VVB, false, true, T, T>), grid, block, 0, s, P,    \
                           static_cast<const TA*>(opA), static_cast<const TB*>(opB), static_cast<T*>(out),              \
                           (T)acc->alpha, (T)acc->beta);                                                                \
    } while (0)
        if (a_f32 && b_f32) {
            if (VA > 1) FE_CONTRACT_ACC_CASE(double, float, float, 4, 4, "contract f32 x f32 -> f64 (16-byte groups)");
            else FE_CONTRACT_ACC_CASE(double, float, float, 1, 1, "contract f32 x f32 -> f64");
        } else if (a_f32) {
            if (VA > 1 && VB > 1) FE_CONTRACT_ACC_CASE(double, float, double, 4, 2, "contract f32 x f64 (16-byte groups)");
            else if (VA > 1) FE_CONTRACT_ACC_CASE(double, float, double, 4, 1, "contract f32 x f64 (A 16-byte groups)");
            else if (VB > 1) FE_CONTRACT_ACC_CASE(double, float, double, 1, 2, "contract f32 x f64 (B 16-byte groups)");
            else FE_CONTRACT_ACC_CASE(double, float, double, 1, 1, "contract f32 x f64");
        } else if (b_f32) {
            if (VA > 1 && VB > 1) FE_CONTRACT_ACC_CASE(double, double, float, 2, 4, "contract f64 x f32 (16-byte groups)");
            else if (VA > 1) FE_CONTRACT_ACC_CASE(double, double, float, 2, 1, "contract f64 x f32 (A 16-byte groups)");
            else if (VB > 1) FE_CONTRACT_ACC_CASE(double, double, float, 1, 4, "contract f64 x f32 (B 16-byte groups)");
            else FE_CONTRACT_ACC_CASE(double, double, float, 1, 1, "contract f64 x f32");
        } else if (f64) {
            if (V > 1) FE_CONTRACT_ACC_CASE(double, double, double, 2, 2, "contract f64 (16-byte groups)");
            else FE_CONTRACT_ACC_CASE(double, double, double, 1, 1, "contract f64");
        } else {
            if (V > 1) FE_CONTRACT_ACC_CASE(float, float, float, 4, 4, "contract f32 (16-byte groups)");
            else FE_CONTRACT_ACC_CASE(float, float, float, 1, 1, "contract f32");
        }
#undef FE_CONTRACT_ACC_CASE
        FE_HIP_CHECK(hipGetLastError());
        return FE_OK;
    }
#define FE_CONTRACT_CASE(T, VV, NAME)                                                                                   \
    do {                                                                                                                \
        static PerDeviceOnce once;                                                                                      \
        if (int rc = configured(once, fe::contract_mfma_kernel<T, VV>, NAME, 0, fe::kCtThreads, fe::kCtBlocksPerCu))   \
            return rc;                                                                                                  \
        hipLaunchKernelGGL((fe::contract_mfma_kernel<T, VV>), grid, block, 0, s, P, static_cast<const T*>(opA),        \
                           static_cast<const T*>(opB), static_cast<T*>(out));                                          \
    } while (0)
#define FE_CONTRACT_MIXED_CASE(TA, TB, VVA, VVB, NAME)                                                          \
    do {                                                                                                                \
        static PerDeviceOnce once;                                                                                      \
        if (int rc = configured(once, fe::contract_mfma_kernel<double, VVA, TA, TB, VVB>, NAME, 0, fe::kCtThreads,       \
                                fe::kCtBlocksPerCu))                                                                    \
            return rc;                                                                                                  \
        hipLaunchKernelGGL((fe::contract_mfma_kernel<double, VVA, TA, TB, VVB>), grid, block, 0, s, P,                    \
                           static_cast<const TA*>(opA), static_cast<const TB*>(opB), static_cast<double*>(out));        \
    } while (0)
    if (a_f32 && b_f32) {
        if (VA > 1) FE_CONTRACT_MIXED_CASE(float, float, 4, 4, "contract f32 x f32 -> f64 (16-byte groups)");
        else FE_CONTRACT_MIXED_CASE(float, float, 1, 1, "contract f32 x f32 -> f64");
    } else if (a_f32) {
        if (VA > 1 && VB > 1) FE_CONTRACT_MIXED_CASE(float, double, 4, 2, "contract f32 x f64 (16-byte groups)");
        else if (VA > 1) FE_CONTRACT_MIXED_CASE(float, double, 4, 1, "contract f32 x f64 (A 16-byte groups)");
        else if (VB > 1) FE_CONTRACT_MIXED_CASE(float, double, 1, 2, "contract f32 x f64 (B 16-byte groups)");
        else FE_CONTRACT_MIXED_CASE(float, double, 1, 1, "contract f32 x f64");
    } else if (b_f32) {
        if (VA > 1 && VB > 1) FE_CONTRACT_MIXED_CASE(double, float, 2, 4, "contract f64 x f32 (16-byte groups)");
        else if (VA > 1) FE_CONTRACT_MIXED_CASE(double, float, 2, 1, "contract f64 x f32 (A 16-byte groups)");
        else if (VB > 1) FE_CONTRACT_MIXED_CASE(double, float, 1, 4, "contract f64 x f32 (B 16-byte groups)");
        else FE_CONTRACT_MIXED_CASE(double, float, 1, 1, "contract f64 x f32");
    } else if (f64) {
        if (V > 1) FE_CONTRACT_CASE(double, 2, "contract f64 (16-byte groups)");
        else FE_CONTRACT_CASE(double, 1, "contract f64");
    } else {
        if (V > 1) FE_CONTRACT_CASE(float, 4, "contract f32 (16-byte groups)");
        else FE_CONTRACT_CASE(float, 1, "contract f32");
    }
#undef FE_CONTRACT_CASE
#undef FE_CONTRACT_MIXED_CASE
    FE_HIP_CHECK(hipGetLastError());
    return FE_OK;
}

int fe_einsum_contract(const fe_einsum_desc* d, const void* const* operands, void* out, void* stream) {
    return contract_launch(d, operands, out, stream, nullptr);
}

int fe_einsum_contract_acc(const fe_einsum_desc* d, const void* const* operands, void* out, double alpha, double beta,
                           void* stream) {
    if (!std::isfinite(alpha) || !std::isfinite(beta))
        return fail(FE_EINVAL, "contract: alpha and beta must be finite (got %g, %g)", alpha, beta);
    const AccScale acc = {alpha, beta};
    return contract_launch(d, operands, out, stream, nullptr, &acc);
}

int fe_einsum_reduce_plan(const fe_einsum_desc* d, int32_t* path, int64_t* slices, size_t* workspace_bytes) {
    if (!path || !slices || !workspace_bytes) return fail(FE_EINVAL, "reduce plan: null pointer");
    ReduceSetup r;
    if (int rc = reduce_setup("reduce plan", d, &r)) return rc;
    *path = r.path;
    *slices = r.slices;
    *workspace_bytes = r.ws_bytes;
    return FE_OK;
}

}  // extern "C"
namespace {
// out[o] = the sum of the `slices` partials of entry o in the workspace (fe_reduce.h), in slice order: the second launch of
// the split reduction and of the operator gradients.  One registration per element type, whoever launches it.
template <typename T>
int launch_reduce_combine(const char* name, const void* workspace, void* out, int64_t n_out, int64_t slices, hipStream_t s) {
    static PerDeviceOnce once;
    if (int rc = configured(once, fe::reduce_combine_kernel<T>, name, 0, fe::kRdThreads, 1)) return rc;
    const dim3 cgrid((unsigned)((n_out + fe::kRdThreads / 64 - 1) / (fe::kRdThreads / 64))), cblock(fe::kRdThreads);
    hipLaunchKernelGGL((fe::reduce_combine_kernel<T>), cgrid, cblock, 0, s, static_cast<const T*>(workspace),
                       static_cast<T*>(out), n_out, slices);
    return FE_OK;
}

// out[o] <- alpha (that sum) + beta out[o]: the second launch of fe_einsum_reduce_acc.
template <typename T>
int launch_reduce_combine_acc(const char* name, const void* workspace, void* out, int64_t n_out, int64_t slices,
                              const AccScale& acc, hipStream_t s) {
    static PerDeviceOnce once;
    if (int rc = configured(once, fe::reduce_combine_kernel<T, true, T, T>, name, 0, fe::kRdThreads, 1)) return rc;
    const dim3 cgrid((unsigned)((n_out + fe::kRdThreads / 64 - 1) / (fe::kRdThreads / 64))), cblock(fe::kRdThreads);
    hipLaunchKernelGGL((fe::reduce_combine_kernel<T, true, T, T>), cgrid, cblock, 0, s, static_cast<const T*>(workspace),
                       static_cast<T*>(out), n_out, slices, (T)acc.alpha, (T)acc.beta);
    return FE_OK;
}

// fe_einsum_reduce, and (acc: not null) fe_einsum_reduce_acc: the partials alike, the accumulating combine launch.
int reduce_launch(const fe_einsum_desc* d, const void* const* operands, void* out, void* workspace,
                  size_t workspace_bytes, void* stream, const AccScale* acc) {
    if (!operands) return fail(FE_EINVAL, "reduce: null operand array");
    ReduceSetup r;
    if (int rc = reduce_setup("reduce", d, &r)) return rc;
    if (r.n_out == 0) return FE_OK;
    if (!out) return fail(FE_EINVAL, "reduce: null output pointer");
    if (reinterpret_cast<uintptr_t>(out) % r.esize) return fail(FE_EINVAL, "reduce: output not aligned to its element size");
    if (!workspace) return fail(FE_EINVAL, "reduce: null workspace (fe_einsum_reduce_plan: %zu bytes)", r.ws_bytes);
    if (workspace_bytes < r.ws_bytes)
        return fail(FE_EINVAL, "reduce: workspace of %zu bytes, the plan needs %zu", workspace_bytes, r.ws_bytes);
    if (reinterpret_cast<uintptr_t>(workspace) % kReduceWsAlign)
        return fail(FE_EINVAL, "reduce: workspace not %zu-byte aligned", kReduceWsAlign);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool f64 = r.esize == 8;
    if (r.path == FE_REDUCE_MFMA) {
        const SplitK split = {r.slices, r.k_slice_len, workspace};
        if (int rc = contract_launch(d, operands, out, stream, &split)) return rc;
    } else {
        fe::ReducePlan& P = r.V;
        fe_einsum_ptrs ops;
        for (int p = 0; p < FE_MAX_EINSUM_OPERANDS; ++p) ops.p[p] = nullptr;
        bool vec = P.n_sum == 1 && P.C == 1;
        for (int p = 0; p < d->n_operands; ++p) {
            const size_t es = (r.f32_mask >> p & 1) ? 4 : r.esize;
            if (!operands[p] && P.n_sum_points > 0) return fail(FE_EINVAL, "reduce: null operand %d", p);
            if (reinterpret_cast<uintptr_t>(operands[p]) % es)
                return fail(FE_EINVAL, "reduce: operand %d not aligned to its element size", p);
            ops.p[p] = operands[p];
            // one vector load per V points: unit stride, every output entry's base a multiple of V, the pointer aligned
            const int64_t Vw = f64 ? 2 : 4;
            if (vec && (P.sum_st[p][0] != 1 || reinterpret_cast<uintptr_t>(operands[p]) % (Vw * es))) vec = false;
            for (int k = 0; k < P.n_out && vec; ++k) vec = P.out_st[p][k] % Vw == 0;
        }
        P.vec = vec;
        const dim3 grid((unsigned)P.slices, (unsigned)r.out_chunks), block(fe::kRdThreads);
#define FE_REDUCE_CASE(T, MIXED, VEC, NAME)                                                                             \
    do {                                                                                                                \
        static PerDeviceOnce once;                                                                                      \
        if (int rc = configured(once, fe::reduce_partial_kernel<T, MIXED, VEC>, NAME, 0, fe::kRdThreads, 1)) return rc; \
        hipLaunchKernelGGL((fe::reduce_partial_kernel<T, MIXED, VEC>), grid, block, 0, s, P, ops,                       \
                           static_cast<T*>(workspace));                                                                 \
    } while (0)
        if (r.f32_mask) {
            if (vec) FE_REDUCE_CASE(double, true, true, "reduce partials mixed (16-byte loads)");
            else FE_REDUCE_CASE(double, true, false, "reduce partials mixed");
        } else if (f64) {
            if (vec) FE_REDUCE_CASE(double, false, true, "reduce partials f64 (16-byte loads)");
            else FE_REDUCE_CASE(double, false, false, "reduce partials f64");
        } else {
            if (vec) FE_REDUCE_CASE(float, false, true, "reduce partials f32 (16-byte loads)");
            else FE_REDUCE_CASE(float, false, false, "reduce partials f32");
        }
#undef FE_REDUCE_CASE
        FE_HIP_CHECK(hipGetLastError());
    }
    if (acc) {
        if (int rc = f64 ? launch_reduce_combine_acc<double>("reduce combine f64 acc", workspace, out, r.n_out, r.slices, *acc, s)
                         : launch_reduce_combine_acc<float>("reduce combine f32 acc", workspace, out, r.n_out, r.slices, *acc, s))
            return rc;
    } else if (int rc = f64 ? launch_reduce_combine<double>("reduce combine f64", workspace, out, r.n_out, r.slices, s)
                            : launch_reduce_combine<float>("reduce combine f32", workspace, out, r.n_out, r.slices, s)) {
        return rc;
    }
    FE_HIP_CHECK(hipGetLastError());
    return FE_OK;
}

}  // namespace
extern "C" {

int fe_einsum_reduce(const fe_einsum_desc* d, const void* const* operands, void* out, void* workspace,
                     size_t workspace_bytes, void* stream) {
    return reduce_launch(d, operands, out, workspace, workspace_bytes, stream, nullptr);
}

int fe_einsum_reduce_acc(const fe_einsum_desc* d, const void* const* operands, void* out, void* workspace,
                         size_t workspace_bytes, double alpha, double beta, void* stream) {
    if (!std::isfinite(alpha) || !std::isfinite(beta))
        return fail(FE_EINVAL, "reduce: alpha and beta must be finite (got %g, %g)", alpha, beta);
    const AccScale acc = {alpha, beta};
    return reduce_launch(d, operands, out, workspace, workspace_bytes, stream, &acc);
}

int fe_einsum_contract_groups(const fe_einsum_desc* d, int32_t* out_group, int32_t* sum_group) {
    if (!d || !out_group || !sum_group) return fail(FE_EINVAL, "contract groups: null pointer");
    if (d->n_operands != 2)
        return fail(FE_EUNSUPPORTED, "contract groups: %d operands (the contraction kernel takes exactly 2)", d->n_operands);
    if (d->n_out < 0 || d->n_out > FE_MAX_EINSUM_INDICES || d->n_sum < 0 || d->n_sum > FE_MAX_EINSUM_INDICES)
        return fail(FE_EINVAL, "contract groups: %d output / %d summation indices out of range", d->n_out, d->n_sum);
    contract_groups(d, out_group, sum_group);
    return FE_OK;
}

#ifdef FE_EXPERIMENTS
int fe_dbg_read_clock(unsigned long long* out2) {
    FE_HIP_CHECK(hipDeviceSynchronize());
    FE_HIP_CHECK(hipMemcpyFromSymbol(out2, HIP_SYMBOL(fe::fe_dbg_clock), 16));
    return FE_OK;
}
int fe_dbg_read_w8(unsigned long long* out, int n_waves) {
    FE_HIP_CHECK(hipDeviceSynchronize());
    FE_HIP_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(fe::fe_dbg_w8), (size_t)n_waves * 64));
    return FE_OK;
}
int fe_dbg_read_phase(unsigned long long* out, int n_waves) {
    FE_HIP_CHECK(hipDeviceSynchronize());
    FE_HIP_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(fe::fe_dbg_phase), (size_t)n_waves * 32));
    return FE_OK;
}
int fe_dbg_read_tiles(unsigned long long* out, int n_waves) {
    FE_HIP_CHECK(hipDeviceSynchronize());
    FE_HIP_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(fe::fe_dbg_tile), (size_t)n_waves * 128));
    return FE_OK;
}
int fe_dbg_read_stamps(unsigned long long* out, int n_waves) {
    FE_HIP_CHECK(hipDeviceSynchronize());
    FE_HIP_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(fe::fe_dbg_stamps), (size_t)n_waves * 32));
    return FE_OK;
}
#endif

int fe_set_tail_rounds(int32_t rounds) {
    const int before = g_tail_rounds.exchange(rounds);
    return before;
}

int fe_set_temporal_loads_mib(int32_t mib) {
    return (int)(g_temporal_input_bytes.exchange(mib < 0 ? 0 : (long long)mib << 20) >> 20);
}

int fe_set_write_through_mib(int32_t mib) {
    return (int)(g_write_through_output_bytes.exchange(mib < 0 ? 0 : (long long)mib << 20) >> 20);
}

int fe_last_launch_info(int64_t* out, int32_t n) {
    if (!out || n < 1) return fail(FE_EINVAL, "fe_last_launch_info: bad arguments");
    const LastLaunch& L = g_last_launch;
    const int64_t v[FE_LAST_LAUNCH_INFO] = {L.valid, L.dynamic_walk, L.temporal_loads, L.write_through, L.blocks, L.waves_per_block, L.kind, L.bodies,
                                            L.tiles, L.static_tiles};
    for (int k = 0; k < n && k < FE_LAST_LAUNCH_INFO; ++k) out[k] = v[k];
    return n < FE_LAST_LAUNCH_INFO ? n : FE_LAST_LAUNCH_INFO;
}

int fe_set_div_quarter_tail(int32_t on) {
    return g_div_quarter_tail.exchange(on ? 1 : 0);
}

int fe_set_grad_quarter_tail(int32_t on) {
    return g_grad_quarter_tail.exchange(on < 0 ? 0 : (on == 2 || on == 3) ? 1 : on);
}

int fe_set_grad_staggered_start(int32_t on) {
    return g_grad_staggered_start.exchange(on ? 1 : 0);
}

int fe_set_tail_min_rounds(int32_t rounds) {
    return g_tail_min_rounds_v.exchange(rounds < 2 ? 2 : rounds);
}

int64_t fe_set_div_interleave(int64_t tiles) {
    return g_div_interleave_tiles.exchange(tiles < 0 ? 0 : tiles);
}

int fe_set_phase_priority_p5(int32_t on) {
    return g_phase_priority_p5.exchange(on ? 1 : 0);
}

int fe_set_cu_limit(int32_t cus) {
    return g_cu_limit.exchange(cus < 0 ? 0 : cus);
}

int fe_stream_retired(void* stream) {
    int dev = 0;
    FE_HIP_CHECK(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) return fail(FE_EINVAL, "fe_stream_retired: device %d", dev);
    TailPool& pool = g_tail[dev];
    std::lock_guard<std::mutex> guard(pool.lock);
    auto it = pool.by_stream.find(tail_stream_key(static_cast<hipStream_t>(stream)));
    if (it == pool.by_stream.end()) return 0;
    pool.spare.push_back(it->second);   // zero, like every group between launches
    pool.verified_at.erase(it->first);
    pool.by_stream.erase(it);
    return 1;
}

int fe_capture_id(void* stream, uint64_t* id) {
    if (!id) return fail(FE_EINVAL, "fe_capture_id: null result pointer");
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    unsigned long long cid = 0;
    FE_HIP_CHECK(hipStreamGetCaptureInfo(static_cast<hipStream_t>(stream), &st, &cid));
    *id = st == hipStreamCaptureStatusNone ? 0 : (uint64_t)cid;
    return FE_OK;
}

int fe_graph_retired(uint64_t capture_id) {
    int dev = 0;
    FE_HIP_CHECK(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) return fail(FE_EINVAL, "fe_graph_retired: device %d", dev);
    TailPool& pool = g_tail[dev];
    std::lock_guard<std::mutex> guard(pool.lock);
    auto it = pool.by_capture.find((unsigned long long)capture_id);
    if (it == pool.by_capture.end()) return 0;
    const int n = (int)it->second.size();
    for (unsigned* g : it->second) pool.spare.push_back(g);   // zero, like every group between launches
    pool.captured -= n;
    pool.by_capture.erase(it);
    return n;
}

int fe_tail_stats(int64_t* out, int32_t n) {
    if (!out || n < 1) return fail(FE_EINVAL, "fe_tail_stats: bad arguments");
    int dev = 0;
    FE_HIP_CHECK(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) return fail(FE_EINVAL, "fe_tail_stats: device %d", dev);
    TailPool& pool = g_tail[dev];
    std::lock_guard<std::mutex> guard(pool.lock);
    const int64_t v[FE_TAIL_STATS] = {pool.groups, (int64_t)pool.by_stream.size(), pool.captured, (int64_t)pool.spare.size(), pool.exhausted,
                                      pool.static_fallbacks, pool.grow_failures, pool.verified_after_error, pool.repaired_after_error,
                                      (int64_t)pool.by_capture.size(), kTailMaxGroups, (int64_t)g_hip_error_epoch.load()};
    for (int k = 0; k < n && k < FE_TAIL_STATS; ++k) out[k] = v[k];
    return n < FE_TAIL_STATS ? n : FE_TAIL_STATS;
}

int fe_tail_plant(void* stream, uint32_t value) {
    int dev = 0;
    FE_HIP_CHECK(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) return fail(FE_EINVAL, "fe_tail_plant: device %d", dev);
    unsigned* group = nullptr;
    {
        TailPool& pool = g_tail[dev];
        std::lock_guard<std::mutex> guard(pool.lock);
        auto it = pool.by_stream.find(tail_stream_key(static_cast<hipStream_t>(stream)));
        if (it == pool.by_stream.end()) return fail(FE_EINVAL, "fe_tail_plant: the stream owns no counter group (no dynamic launch yet)");
        group = it->second;
    }
    FE_HIP_CHECK(hipDeviceSynchronize());
    FE_HIP_CHECK(hipMemcpy(group + 3 * fe::kTailStride, &value, sizeof(value), hipMemcpyHostToDevice));   // pool 3's ticket counter
    return FE_OK;
}

int fe_tail_check(int32_t repair, int64_t* dirty_words, int32_t* groups, int32_t* streams, int32_t* captured) {
    int dev = 0;
    FE_HIP_CHECK(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) return fail(FE_EINVAL, "fe_tail_check: device %d", dev);
    FE_HIP_CHECK(hipDeviceSynchronize());
    TailPool& pool = g_tail[dev];
    std::lock_guard<std::mutex> guard(pool.lock);
    long long dirty = 0;
    for (unsigned* chunk : pool.chunks)
        for (int g = 0; g < kTailChunkGroups; ++g)
            if (int rc = tail_group_dirty(chunk + (size_t)g * kTailGroupWords, repair != 0, &dirty)) return rc;
    if (dirty_words) *dirty_words = dirty;
    if (groups) *groups = pool.groups;
    if (streams) *streams = (int32_t)pool.by_stream.size();
    if (captured) *captured = pool.captured;
    return FE_OK;
}

int fe_launch_f32(int32_t family, const fe_argpack* a, void* stream) {
    forget_last_launch();
    if (!a) return fail(FE_EINVAL, "fe_launch_f32: null argument pack");
    if (a->E < 0 || a->Np <= 0) return fail(FE_EINVAL, "fe_launch_f32: bad sizes (E=%lld Np=%d)", (long long)a->E, a->Np);
    if (a->E == 0) return FE_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int ndim = a->ndim == 2 ? 2 : 3;
    PackFields fields;
    if (int rc = pack_fields("fe_launch_f32", a, &fields)) return rc;
    const int b = fields.b;
    const double* const* vin = reinterpret_cast<const double* const*>(fields.in);
    double* const* vout = fields.out;
    int opT = 0, jl = 0, rl = 0, nf = 0, Nfp = 0;
    switch (family) {
        case FE_FAMILY_GRAD:
        case FE_FAMILY_DIV:
        case FE_FAMILY_MATAPPLY:
            if (a->layout_flags & ~FE_OP_TRANSPOSED) return fail(FE_EINVAL, "fe_launch_f32: bad operator flags %d", a->layout_flags);
            opT = (a->layout_flags & FE_OP_TRANSPOSED) ? 1 : 0;
            break;
        case FE_FAMILY_DIVCOMP:
            if (a->layout_flags & ~(FE_OP_TRANSPOSED | FE_OP_J_ES)) return fail(FE_EINVAL, "fe_launch_f32: bad operator flags %d", a->layout_flags);
            opT = (a->layout_flags & FE_OP_TRANSPOSED) ? 1 : 0;
            jl = (a->layout_flags & FE_OP_J_ES) ? 1 : 0;
            break;
        case FE_FAMILY_FACEMASS: {
            if (a->nf <= 0 || a->Nfp <= 0) return fail(FE_EINVAL, "fe_launch_f32: face-mass needs nf and Nfp");
            nf = a->nf;
            Nfp = a->Nfp;
            const fe::FmLayout L(a->layout_flags, a->Np, nf, Nfp, a->E);
            jl = L.jfe;
            rl = L.rifj;
            break;
        }
        default:
            return fail(FE_EUNSUPPORTED, "fe_launch_f32: family %d has no float32 kernel", family);
    }
    if (!a->D || (family != FE_FAMILY_MATAPPLY && !a->J)) return fail(FE_EINVAL, "fe_launch_f32: null device pointer");
    // tetrahedra p = 1 ... 4 on the matrix cores (fe_grad_f32.h, fe_div_f32.h, fe_facemass_f32.h): 16-byte aligned operands, E a
    // multiple of 4 (so that every row of J and every plane starts on a 16-byte boundary) and at least one full wave tile; else
    // the tiled kernel.  The dispatches on Np below are the one list of shapes that have such a kernel: any other leaves rc = 1.
    const bool tets = family == FE_FAMILY_FACEMASS ? nf == 4 : (family == FE_FAMILY_GRAD || family == FE_FAMILY_DIV) && ndim == 3;
    if (tets && a->variant != FE_VARIANT_TILED && a->E % 4 == 0 && a->E >= 16) {
        bool aligned = ((reinterpret_cast<uintptr_t>(a->J) | reinterpret_cast<uintptr_t>(a->D)) & 15u) == 0;
        for (int k = 0; k < b; ++k)
            aligned = aligned && vin[k] && vout[k] && ((reinterpret_cast<uintptr_t>(vin[k]) | reinterpret_cast<uintptr_t>(vout[k])) & 15u) == 0;
        int rc = 1;   // 1: no MFMA launch (no kernel for the shape, unaligned, or too few elements for a wave tile): the tiled kernel below
        if (!aligned) {
        } else if (family == FE_FAMILY_DIV) {   // the kernel over the geometry (Np, M) of the float64 div
            if (fe::is_tet_order(a->Np))
                rc = fe::with_tet_order(a->Np, [&](auto o) {
                    using O = decltype(o);
                    static const What what(O::NP == 35 ? "div float32 Np=%d" : "div float32 Np=%d M=%d", O::NP, O::MD);
                    return launch_f32_fields<fe::DivF32GeomT<O::NP, O::MD>, fe::div3d_mfma_f32_kernel<O::NP, O::MD>>(a, vin, vout, b, opT, what, s);
                });
        } else if (family == FE_FAMILY_FACEMASS) {   // the kernel over the geometry (Np, Nfp, M) of the float64 face-mass
            if (fe::is_tet_order(a->Np, Nfp))
                rc = fe::with_tet_order(a->Np, [&](auto o) {
                    using O = decltype(o);
                    static const What what(O::NP == 35 ? "face-mass float32 Np=%d" : "face-mass float32 Np=%d M=%d", O::NP, O::MF);
                    return launch_f32_facemass<fe::FmF32GeomT<O::NP, O::NFP, O::MF>, fe::facemass_mfma_f32_kernel<O::NP, O::NFP, O::MF>>(
                        a, vin, vout, b, jl, rl, what, s);
                });
        } else {
            // two 16-element sub-tiles per wave iteration from E = 2e5 on (round 4: 4.5 KB store bursts, two blocks per CU: 68.1 ->
            // 70.5 % of the float32 roofline at 1e6, 70.2 -> 75.5 % at 4e6; below 2e5 the three-blocks-per-CU kernel of one sub-tile
            // is faster: 15.3 against 17.7 us at 1e5; FEINSUM_F32_M=1 / 2 forces either; profiles/r04/float32_grad_two_subtiles.txt)
            static const int m_env = [] { const char* e = getenv("FEINSUM_F32_M"); return e ? atoi(e) : 0; }();
            const bool m1 = m_env == 1 || (m_env != 2 && a->E < 200000);
            const int flags = opT | temporal_flag((9 + (int64_t)a->Np) * a->E * 4);
            // behind two static rounds the tiles come by tickets (from five rounds on, as for float64) -- not on the one-sub-tile kernel
            rc = a->Np == 35 ? (m1 ? launch_f32_fields<fe::GradF32GeomT<1>, fe::grad3d_mfma_f32_kernel<1>>(a, vin, vout, b, flags, "grad float32 Np=35 M=1", s)
                                   : launch_f32_fields<fe::GradF32GeomT<2>, fe::grad3d_mfma_f32_kernel<2>, fe::grad3d_mfma_f32_tail_kernel<2>>(
                                         a, vin, vout, b, flags, "grad float32 Np=35 M=2", s))
                 : a->Np == 20 ? launch_f32_fields<fe::GradF32GeomT<3, 20>, fe::grad3d_mfma_f32_kernel<3, 20>, fe::grad3d_mfma_f32_tail_kernel<3, 20>>(
                                     a, vin, vout, b, flags, "grad float32 Np=20 M=3", s)
                 : a->Np == 10 ? launch_f32_fields<fe::GradF32GeomT<5, 10>, fe::grad3d_mfma_f32_kernel<5, 10>, fe::grad3d_mfma_f32_tail_kernel<5, 10>>(
                                     a, vin, vout, b, flags, "grad float32 Np=10 M=5", s)
                 : a->Np == 4 ? launch_f32_fields<fe::GradF32GeomT<8, 4>, fe::grad3d_mfma_f32_kernel<8, 4>, fe::grad3d_mfma_f32_tail_kernel<8, 4>>(
                                    a, vin, vout, b, flags, "grad float32 Np=4 M=8", s)
                              : 1;
        }
        if (rc <= 0) return rc;
    }
    // groups of up to kMaxFields fields share the staged operator; a div component is one launch of one field, whatever b
    // says (the pointers of its first group are still checked)
    const int walked = family == FE_FAMILY_DIVCOMP && b > fe::kMaxFields ? fe::kMaxFields : b;
    return fe::for_each_field_group(walked, fe::kMaxFields, false, [&](int k0, int nb) {
        fe::FieldPtrs P = {};
        for (int k = 0; k < nb; ++k) {
            if (!vin[k0 + k] || !vout[k0 + k]) return fail(FE_EINVAL, "fe_launch_f32: null field pointer");
            P.v[k] = vin[k0 + k];
            P.out[k] = vout[k0 + k];
        }
        const fe::TiledArgs ta = tiled_args(family, a->J, a->D, P, family == FE_FAMILY_DIVCOMP ? 1 : nb, a->E,
                                            family == FE_FAMILY_MATAPPLY ? 1 : ndim, a->Np, nf, Nfp, opT, jl, rl);
        return launch_tiled_t<float>(ta, s);
    });
}

// float32 fields, float64 J / operator / outputs (fe_mixed.h)
int fe_div3d_mixed_f64(const double* J, const double* D, const void* const* fields, double* const* outs, int64_t E, int32_t Np,
                       int32_t b, int32_t layout_flags, void* stream) {
    forget_last_launch();
    const float* const* v = reinterpret_cast<const float* const*>(fields);
    CallCheck c = {"div, float32 fields", J, D, fields, ptr_table(outs), E, Np, b, layout_flags, FE_OP_TRANSPOSED};
    c.in_align = 4;
    c.scope = kScopeTet;
    FE_CHECK_CALL(c);
    bool plain = false;   // a plane x E Np floats behind a field's start that is not on an 8-byte boundary: no LDS-DMA for the fields
    for (int k = 0; k < b; ++k)
        for (int x = 0; x < 3; ++x) plain = plain || ((reinterpret_cast<uintptr_t>(v[k]) + (uintptr_t)x * (uintptr_t)E * Np * 4u) & 7u) != 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int opT = (layout_flags & FE_OP_TRANSPOSED) ? 1 : 0;
    return fe::with_tet_order(Np, [&](auto o) {
        using O = decltype(o);
        static const What what("div float32 fields Np=%d M=%d", O::NP, O::MD),
            what_plain("div float32 fields Np=%d M=%d, plain loads", O::NP, O::MD);
        return launch_mixed_fields<fe::DivMixedGeomT<O::NP, O::MD>, fe::div3d_mixed_kernel<O::NP, O::MD, false>,
                                   fe::div3d_mixed_kernel<O::NP, O::MD, true>>(J, D, v, outs, b, E, opT, plain, what, what_plain, s);
    });
}

int fe_grad3d_mixed_f64(const double* J, const double* D, const void* const* fields, double* const* outs, int64_t E, int32_t Np,
                        int32_t b, int32_t layout_flags, void* stream) {
    forget_last_launch();
    const float* const* v = reinterpret_cast<const float* const*>(fields);
    CallCheck c = {"grad, float32 fields", J, D, fields, ptr_table(outs), E, Np, b, layout_flags, FE_OP_TRANSPOSED};
    c.in_align = 4;
    c.scope = kScopeTet;
    FE_CHECK_CALL(c);
    bool plain = false;   // a field that does not start on an 8-byte boundary: no LDS-DMA for the fields
    for (int k = 0; k < b; ++k) plain = plain || (reinterpret_cast<uintptr_t>(v[k]) & 7u) != 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int opT = (layout_flags & FE_OP_TRANSPOSED) ? 1 : 0;
    return fe::with_tet_order(Np, [&](auto o) {
        using O = decltype(o);
        static const What what("grad float32 fields Np=%d M=%d", O::NP, O::MG),
            what_plain("grad float32 fields Np=%d M=%d, plain loads", O::NP, O::MG);
        return launch_mixed_fields<fe::GradMixedGeomT<O::MG, O::NP>, fe::grad3d_mixed_kernel<O::MG, O::NP, false>,
                                   fe::grad3d_mixed_kernel<O::MG, O::NP, true>>(J, D, v, outs, b, E, opT, plain, what, what_plain, s);
    });
}

int fe_facemass_mixed_f64(const double* J, const double* R, const void* const* fields, double* const* outs, int64_t E, int32_t Np,
                          int32_t nf, int32_t Nfp, int32_t b, int32_t layout_flags, void* stream) {
    forget_last_launch();
    const float* const* v = reinterpret_cast<const float* const*>(fields);
    CallCheck c = {"face-mass, float32 fields", J, R, fields, ptr_table(outs), E, Np, b, layout_flags, 7};
    c.flag_name = "layout";
    c.in_align = 4;
    c.faces = true; c.nf = nf; c.Nfp = Nfp;
    c.scope = kScopeTetFaces;
    FE_CHECK_CALL(c);
    bool plain = false;   // a face slab f E Nfp floats behind a field's start that is not on an 8-byte boundary
    for (int k = 0; k < b; ++k)
        for (int f = 0; f < 4; ++f) plain = plain || ((reinterpret_cast<uintptr_t>(v[k]) + (uintptr_t)f * (uintptr_t)E * Nfp * 4u) & 7u) != 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const fe::FmLayout L(layout_flags, Np, nf, Nfp, E);
    return fe::with_tet_order(Np, [&](auto o) {
        using O = decltype(o);
        static const What what("face-mass float32 fields Np=%d M=%d", O::NP, O::MF),
            what_plain("face-mass float32 fields Np=%d M=%d, plain loads", O::NP, O::MF);
        return launch_mixed_facemass<fe::FmMixedGeomT<O::NP, O::NFP, O::MF>, fe::facemass_mixed_kernel<O::NP, O::NFP, O::MF, false>,
                                     fe::facemass_mixed_kernel<O::NP, O::NFP, O::MF, true>>(J, R, v, outs, b, E, L.jfe, L.rifj, plain, what,
                                                                                            what_plain, s);
    });
}

// float32 fields and float32 results, float64 J / operator / arithmetic (fe_mixed.h, OUT = float).  The store form of a launch:
// 16 bytes per lane when every output plane starts on an 8-byte boundary, else one float per lane.
int fe_div3d_mixed_state_f64(const double* J, const double* D, const void* const* fields, void** outs, int64_t E, int32_t Np,
                             int32_t b, int32_t layout_flags, void* stream) {
    forget_last_launch();
    const float* const* v = reinterpret_cast<const float* const*>(fields);
    float* const* o = reinterpret_cast<float* const*>(outs);
    CallCheck c = {"div, float32 fields and results", J, D, fields, ptr_table(outs), E, Np, b, layout_flags, FE_OP_TRANSPOSED};
    c.in_align = c.out_align = 4;
    c.scope = kScopeTet; c.scope_first = true;
    FE_CHECK_CALL(c);
    bool plain = false, dwords = false;   // (the rules of fe_div3d_mixed_f64; the outputs have one plane each)
    for (int k = 0; k < b; ++k) {
        for (int x = 0; x < 3; ++x) plain = plain || ((reinterpret_cast<uintptr_t>(v[k]) + (uintptr_t)x * (uintptr_t)E * Np * 4u) & 7u) != 0;
        dwords = dwords || (reinterpret_cast<uintptr_t>(o[k]) & 7u) != 0;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int op_flags = ((layout_flags & FE_OP_TRANSPOSED) ? 1 : 0) | (dwords ? fe::kOpDwordStores : 0);
    return fe::with_tet_order(Np, [&](auto o_) {
        using O = decltype(o_);
        static const What what("div float32 fields+results Np=%d M=%d", O::NP, O::MD),
            what_plain("div float32 fields+results Np=%d M=%d, plain loads", O::NP, O::MD);
        return launch_mixed_fields<fe::DivMixedGeomT<O::NP, O::MD, float>, fe::div3d_mixed_kernel<O::NP, O::MD, false, float>,
                                   fe::div3d_mixed_kernel<O::NP, O::MD, true, float>, float>(J, D, v, o, b, E, op_flags, plain, what,
                                                                                            what_plain, s, fe::kLaunchFloat32Results | (dwords ? fe::kLaunchDwordStores : 0));
    });
}

int fe_grad3d_mixed_state_f64(const double* J, const double* D, const void* const* fields, void** outs, int64_t E, int32_t Np,
                              int32_t b, int32_t layout_flags, void* stream) {
    forget_last_launch();
    const float* const* v = reinterpret_cast<const float* const*>(fields);
    float* const* o = reinterpret_cast<float* const*>(outs);
    CallCheck c = {"grad, float32 fields and results", J, D, fields, ptr_table(outs), E, Np, b, layout_flags, FE_OP_TRANSPOSED};
    c.in_align = c.out_align = 4;
    c.scope = kScopeTet; c.scope_first = true;
    FE_CHECK_CALL(c);
    bool plain = false, dwords = ((uint64_t)E * (uint64_t)Np) % 2 != 0;   // planes x E Np floats behind an output's start
    for (int k = 0; k < b; ++k) {
        plain = plain || (reinterpret_cast<uintptr_t>(v[k]) & 7u) != 0;
        dwords = dwords || (reinterpret_cast<uintptr_t>(o[k]) & 7u) != 0;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int op_flags = ((layout_flags & FE_OP_TRANSPOSED) ? 1 : 0) | (dwords ? fe::kOpDwordStores : 0);
    return fe::with_tet_order(Np, [&](auto o_) {
        using O = decltype(o_);
        static const What what("grad float32 fields+results Np=%d M=%d", O::NP, O::MG),
            what_plain("grad float32 fields+results Np=%d M=%d, plain loads", O::NP, O::MG);
        return launch_mixed_fields<fe::GradMixedGeomT<O::MG, O::NP, float>, fe::grad3d_mixed_kernel<O::MG, O::NP, false, float>,
                                   fe::grad3d_mixed_kernel<O::MG, O::NP, true, float>, float>(J, D, v, o, b, E, op_flags, plain, what,
                                                                                             what_plain, s, fe::kLaunchFloat32Results | (dwords ? fe::kLaunchDwordStores : 0));
    });
}

int fe_facemass_mixed_state_f64(const double* J, const double* R, const void* const* fields, void** outs, int64_t E, int32_t Np,
                                int32_t nf, int32_t Nfp, int32_t b, int32_t layout_flags, void* stream) {
    forget_last_launch();
    const float* const* v = reinterpret_cast<const float* const*>(fields);
    CallCheck c = {"face-mass, float32 fields and results", J, R, fields, ptr_table(outs), E, Np, b, layout_flags, 7};
    c.flag_name = "layout";
    c.in_align = c.out_align = 4;
    c.faces = true; c.nf = nf; c.Nfp = Nfp;
    c.scope = kScopeTetFaces; c.scope_first = true;
    FE_CHECK_CALL(c);
    bool plain = false, dwords = false;   // (the rule of fe_facemass_mixed_f64; the outputs have one plane each)
    for (int k = 0; k < b; ++k) {
        for (int f = 0; f < 4; ++f) plain = plain || ((reinterpret_cast<uintptr_t>(v[k]) + (uintptr_t)f * (uintptr_t)E * Nfp * 4u) & 7u) != 0;
        dwords = dwords || (reinterpret_cast<uintptr_t>(outs[k]) & 7u) != 0;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const fe::FmLayout L(layout_flags, Np, nf, Nfp, E);
    return fe::with_tet_order(Np, [&](auto o_) {
        using O = decltype(o_);
        static const What what("face-mass float32 fields+results Np=%d M=%d", O::NP, O::MF),
            what_plain("face-mass float32 fields+results Np=%d M=%d, plain loads", O::NP, O::MF);
        // (the field tables are untyped in FieldPtrs: the kernel reads P.out as float*)
        return launch_mixed_facemass<fe::FmMixedGeomT<O::NP, O::NFP, O::MF, float>, fe::facemass_mixed_kernel<O::NP, O::NFP, O::MF, false, float>,
                                     fe::facemass_mixed_kernel<O::NP, O::NFP, O::MF, true, float>>(
            J, R, v, reinterpret_cast<double* const*>(outs), b, E, L.jfe | (dwords ? fe::kOpDwordStores : 0), L.rifj, plain, what,
            what_plain, s, fe::kLaunchFloat32Results | (dwords ? fe::kLaunchDwordStores : 0));
    });
}

int fe_launch(int32_t family, const fe_argpack* a, void* stream) {
    if (!a) return fail(FE_EINVAL, "fe_launch: null argument pack");
    if (family & FE_FAMILY_FIELDS_F32) {   // float32 fields, everything else float64: the pack's field pointers are nominal
        const int32_t base = family & ~FE_FAMILY_FIELDS_F32;
        if (base != FE_FAMILY_GRAD && base != FE_FAMILY_DIV && base != FE_FAMILY_FACEMASS)
            return fail(FE_EUNSUPPORTED, "fe_launch: family 0x%x has no kernel for float32 fields (float64 grad, div and face-mass "
                        "of tetrahedra; not together with FE_FAMILY_F32 or FE_FAMILY_ACC)", base);
        PackFields f;
        if (int rc = pack_fields("fe_launch", a, &f)) return rc;
        if (base == FE_FAMILY_GRAD) return fe_grad3d_mixed_f64(a->J, a->D, f.in, f.out, a->E, a->Np, f.b, a->layout_flags, stream);
        if (base == FE_FAMILY_DIV) return fe_div3d_mixed_f64(a->J, a->D, f.in, f.out, a->E, a->Np, f.b, a->layout_flags, stream);
        return fe_facemass_mixed_f64(a->J, a->D, f.in, f.out, a->E, a->Np, a->nf, a->Nfp, f.b, a->layout_flags, stream);
    }
    if (family & FE_FAMILY_ACC) {   // out <- alpha * E + beta * out
        const int32_t base = family & ~FE_FAMILY_ACC;
        if (base == FE_FAMILY_FACEMASS)
            return fe_facemass_acc_f64(a->J, a->D, a->v, a->outs, a->E, a->Np, a->nf, a->Nfp, a->b, a->layout_flags, a->alpha,
                                       a->beta, stream);
        if (base != FE_FAMILY_GRAD && base != FE_FAMILY_DIV)
            return fail(FE_EUNSUPPORTED, "fe_launch: family 0x%x has no accumulating kernel (float64 face-mass, grad, div)", base);
        if (!a->v || !a->outs) return fail(FE_EINVAL, "fe_launch: accumulating grad / div take their fields from v / outs");
        for (int k = 0; k < a->b; ++k)   // one accumulating launch per field
            if (int rc = (base == FE_FAMILY_GRAD ? fe_grad3d_acc_f64 : fe_div3d_acc_f64)(
                    a->J, a->D, a->v[k], a->outs[k], a->E, a->Np, a->layout_flags, a->alpha, a->beta, stream))
                return rc;
        return FE_OK;
    }
    if (family & FE_FAMILY_F32) return fe_launch_f32(family & ~FE_FAMILY_F32, a, stream);
    switch (family) {
        case FE_FAMILY_GRAD:
            if (a->ndim == 2)
                return fe_grad_f64(a->J, a->D, a->v, a->outs, a->E, 2, a->Np, a->b, a->layout_flags, a->variant, stream);
            if (a->b > 1)
                return fe_grad3d_prepared_f64(a->J, a->D, a->prepared, a->v, a->outs, a->E, a->Np, a->b, a->layout_flags,
                                              a->variant, stream);
            return fe_grad3d_prepared_f64(a->J, a->D, a->prepared, &a->u, &a->out, a->E, a->Np, 1, a->layout_flags,
                                          a->variant, stream);
        case FE_FAMILY_DIV:
            if (a->ndim == 2)
                return fe_div_f64(a->J, a->D, a->v, a->outs, a->E, 2, a->Np, a->b, a->layout_flags, a->variant, stream);
            if (a->b > 1)
                return fe_div3d_prepared_f64(a->J, a->D, a->prepared, a->v, a->outs, a->E, a->Np, a->b, a->layout_flags,
                                             a->variant, stream);
            return fe_div3d_prepared_f64(a->J, a->D, a->prepared, &a->u, &a->out, a->E, a->Np, 1, a->layout_flags,
                                         a->variant, stream);
        case FE_FAMILY_GRADPLANES:
            return fe_gradplanes3d_f64(a->j3, a->D, a->v, a->outs, a->E, a->Np, a->b, a->layout_flags,
                                       a->variant, stream);
        case FE_FAMILY_MATAPPLY:
            return fe_matapply_f64(a->J, a->D, a->v, a->outs, a->E, a->Np, a->b, a->layout_flags, a->variant,
                                   stream);
        case FE_FAMILY_GRADDIV:
            return fe_graddiv3d_prepared_f64(a->J, a->D, a->prepared, a->u, a->v_div, a->out, a->out2, a->E, a->Np,
                                             a->variant, stream);
        case FE_FAMILY_DIVCOMP:
            return fe_divcomp_f64(a->J, a->D, a->u, a->out, a->E, a->ndim == 2 ? 2 : 3, a->Np, a->layout_flags, a->variant,
                                  stream);
        case FE_FAMILY_FACEMASS:
            return fe_facemass_prepared_f64(a->J, a->D, a->prepared, a->v, a->outs, a->E, a->Np, a->nf, a->Nfp, a->b,
                                            a->layout_flags, a->variant, stream);
        default: return fail(FE_EINVAL, "fe_launch: unknown family %d", family);
    }
}

int fe_time_launches(int32_t family, const fe_argpack* args, int32_t n_launches, void* stream,
                     float* ms_out) {
    if (!args || !ms_out || n_launches <= 0)
        return fail(FE_EINVAL, "fe_time_launches: bad arguments");
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipEvent_t t0, t1;
    FE_HIP_CHECK(hipEventCreate(&t0));
    FE_HIP_CHECK(hipEventCreate(&t1));
    int rc = FE_OK;
    hipError_t e = hipEventRecord(t0, s);
    for (int i = 0; i < n_launches && rc == FE_OK && e == hipSuccess; ++i)
        rc = fe_launch(family, args, stream);
    if (e == hipSuccess) e = hipEventRecord(t1, s);
    if (e == hipSuccess) e = hipEventSynchronize(t1);
    if (e == hipSuccess && rc == FE_OK) e = hipEventElapsedTime(ms_out, t0, t1);
    hipEventDestroy(t0);
    hipEventDestroy(t1);
    if (rc != FE_OK) return rc;
    if (e != hipSuccess) return fail(FE_EHIP, "fe_time_launches: %s", hipGetErrorString(e));
    return FE_OK;
}

}  // extern "C"

// ---- adjoint kernels (fe_adjoint.h) ----
namespace {

template <int NP>
int launch_geomadj(const fe::GeomAdjArgs& g, hipStream_t s) {
    using G = fe::GeomAdjGeom<NP>;
    const int lds = g.R * G::LDS_DOUBLES_PER_R * (int)sizeof(double);
    static PerDeviceOnce once;   // LDS attribute sized for R = 3; the residency is checked at the largest R
    if (int rc = configured(once, fe::geomadj_kernel<NP>, "geomadj", 3 * G::LDS_DOUBLES_PER_R * (int)sizeof(double),
                            fe::kAdjThreads, 2))
        return rc;
    const int64_t n_tiles = (g.E + 15) / 16;
    const unsigned grid = persistent_grid(n_tiles, fe::kAdjWaves);
    hipLaunchKernelGGL(fe::geomadj_kernel<NP>, dim3(grid), dim3(fe::kAdjThreads), lds, s, g);
    FE_HIP_CHECK(hipGetLastError());
    return FE_OK;
}

template <int NP, int NFP, int NF>
int launch_facemass_adj(const fe::FmAdjArgs& g, hipStream_t s) {
    using G = fe::FmAdjGeom<NP, NFP, NF>;
    const int lds = G::LDS_DOUBLES * (int)sizeof(double);
    static PerDeviceOnce once;
    if (int rc = configured(once, fe::facemass_adj_kernel<NP, NFP, NF>, "facemass adjoint", lds, fe::kAdjThreads, 2))
        return rc;
    const int64_t n_tiles = (g.E + 15) / 16;
    const unsigned grid = persistent_grid(n_tiles, fe::kAdjWaves);
    hipLaunchKernelGGL((fe::facemass_adj_kernel<NP, NFP, NF>), dim3(grid), dim3(fe::kAdjThreads), lds, s, g);
    FE_HIP_CHECK(hipGetLastError());
    return FE_OK;
}

bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

}  // namespace

extern "C" {

int fe_geomadj_f64(const double* D, const double* a, const double* b, double* out, int64_t E, int32_t X, int32_t R,
                   int32_t Np, int32_t op_flags, int64_t sx, int64_t sr, int64_t se, void* stream) {
    if (E < 0) return fail(FE_EINVAL, "geomadj: E must be >= 0 (got %lld)", (long long)E);
    if (X < 1 || X > 3 || R < 1 || R > 3) return fail(FE_EUNSUPPORTED, "geomadj: X = %d, R = %d not compiled (1..3)", X, R);
    if (op_flags & ~FE_OP_TRANSPOSED) return fail(FE_EINVAL, "geomadj: bad operator flags %d", op_flags);
    if (E > 0 && (!D || !a || !b || !out)) return fail(FE_EINVAL, "geomadj: null device pointer");
    if (!aligned8(D) || !aligned8(a) || !aligned8(b) || !aligned8(out))
        return fail(FE_EINVAL, "geomadj: device pointers must be 8-byte aligned (float64 arrays)");
    if (E * (int64_t)(Np > 0 ? Np : 1) * X >= (int64_t)1 << 39) return fail(FE_EINVAL, "geomadj: E too large");
    fe::GeomAdjArgs g = {D, a, b, out, E, sx, sr, se, X, R, (op_flags & FE_OP_TRANSPOSED) ? 1 : 0};
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc;
    switch (Np) {
        case 3: rc = E ? launch_geomadj<3>(g, s) : FE_OK; break;
        case 4: rc = E ? launch_geomadj<4>(g, s) : FE_OK; break;
        case 6: rc = E ? launch_geomadj<6>(g, s) : FE_OK; break;
        case 10: rc = E ? launch_geomadj<10>(g, s) : FE_OK; break;
        case 15: rc = E ? launch_geomadj<15>(g, s) : FE_OK; break;
        case 20: rc = E ? launch_geomadj<20>(g, s) : FE_OK; break;
        case 21: rc = E ? launch_geomadj<21>(g, s) : FE_OK; break;
        case 35: rc = E ? launch_geomadj<35>(g, s) : FE_OK; break;
        default: return fail(FE_EUNSUPPORTED, "geomadj: Np = %d not compiled (3, 4, 6, 10, 15, 20, 21, 35)", Np);
    }
    return rc;
}

int fe_facemass_adj_f64(const double* J, const double* R, const double* const* g, const double* const* v,
                        double* const* dv, double* dJ, int64_t E, int32_t Np, int32_t nf, int32_t Nfp, int32_t b,
                        int32_t layout_flags, void* stream) {
    if (E < 0) return fail(FE_EINVAL, "facemass adjoint: E must be >= 0 (got %lld)", (long long)E);
    if (b < 1) return fail(FE_EINVAL, "facemass adjoint: b=%d, need at least one field", b);
    if (!g) return fail(FE_EINVAL, "facemass adjoint: null pointer table");
    if (layout_flags & ~(FE_FM_J_FE | FE_FM_R_IFJ | FE_FM_R_T))
        return fail(FE_EINVAL, "facemass adjoint: bad layout flags %d", layout_flags);
    const bool with_dv = dv != nullptr, with_dJ = v != nullptr && dJ != nullptr;
    if (E > 0 && !with_dv && !with_dJ) return fail(FE_EINVAL, "facemass adjoint: neither dv nor (v, dJ) given");
    int kind = -1;   // compiled shapes
    if (nf == 4 && Np == 4 && Nfp == 3) kind = 0;
    else if (nf == 4 && Np == 10 && Nfp == 6) kind = 1;
    else if (nf == 4 && Np == 20 && Nfp == 10) kind = 2;
    else if (nf == 4 && Np == 35 && Nfp == 15) kind = 3;
    else if (nf == 3 && Np == 3 && Nfp == 2) kind = 4;
    else if (nf == 3 && Np == 6 && Nfp == 3) kind = 5;
    else if (nf == 3 && Np == 10 && Nfp == 4) kind = 6;
    else if (nf == 3 && Np == 15 && Nfp == 5) kind = 7;
    else if (nf == 3 && Np == 21 && Nfp == 6) kind = 8;
    if (kind < 0)
        return fail(FE_EUNSUPPORTED, "facemass adjoint: (nf, Np, Nfp) = (%d, %d, %d) not compiled", nf, Np, Nfp);
    if (E > 0) {
        if (!R || (with_dv && !J)) return fail(FE_EINVAL, "facemass adjoint: null device pointer");
        for (int k = 0; k < b; ++k)
            if (!g[k] || (with_dv && !dv[k]) || (with_dJ && !v[k]))
                return fail(FE_EINVAL, "facemass adjoint: null device pointer (field %d)", k);
    }
    if (!aligned8(J) || !aligned8(R) || !aligned8(dJ)) return fail(FE_EINVAL, "facemass adjoint: device pointers must be 8-byte aligned");
    for (int k = 0; k < b; ++k)
        if (!aligned8(g[k]) || (with_dv && !aligned8(dv[k])) || (with_dJ && !aligned8(v[k])))
            return fail(FE_EINVAL, "facemass adjoint: device pointers must be 8-byte aligned");
    if (E * (int64_t)Np * b >= (int64_t)1 << 39) return fail(FE_EINVAL, "facemass adjoint: E too large");
    if (E == 0) return FE_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // R's strides of (f, i, j): 'fij', 'ifj', 'fji', 'jfi' (as the face-mass kernels read it)
    const fe::FmLayout L(layout_flags, Np, nf, Nfp, E);
    // FE_MAX_FIELDS fields per launch; dJ accumulates over launches
    return fe::for_each_field_group(b, FE_MAX_FIELDS, false, [&](int k0, int nb) {
        fe::FmAdjArgs a = {};
        a.J = J;
        a.R = R;
        for (int k = 0; k < nb; ++k) {
            a.g.v[k] = g[k0 + k];
            a.g.out[k] = with_dv ? dv[k0 + k] : nullptr;
            a.v.v[k] = with_dJ ? v[k0 + k] : nullptr;
        }
        a.dJ = with_dJ ? dJ : nullptr;
        a.E = E;
        a.sje = L.jEs;
        a.sjf = L.jFs;
        a.sF = L.rF, a.sI = L.rI, a.sJ = L.rJ;
        a.nb = nb;
        a.with_dv = with_dv ? 1 : 0;
        a.accumulate = k0 > 0 ? 1 : 0;
        int rc;
        switch (kind) {
            case 0: rc = launch_facemass_adj<4, 3, 4>(a, s); break;
            case 1: rc = launch_facemass_adj<10, 6, 4>(a, s); break;
            case 2: rc = launch_facemass_adj<20, 10, 4>(a, s); break;
            case 3: rc = launch_facemass_adj<35, 15, 4>(a, s); break;
            case 4: rc = launch_facemass_adj<3, 2, 3>(a, s); break;
            case 5: rc = launch_facemass_adj<6, 3, 3>(a, s); break;
            case 6: rc = launch_facemass_adj<10, 4, 3>(a, s); break;
            case 7: rc = launch_facemass_adj<15, 5, 3>(a, s); break;
            default: rc = launch_facemass_adj<21, 6, 3>(a, s); break;
        }
        return rc;
    });
}

}  // extern "C"

// ---- operator gradients (fe_opgrad.h) ----
namespace {

constexpr int64_t kOgMinSlice = 64;      // elements: a slice is at least this long (before rounding to 16)
constexpr int64_t kOgMaxSlices = 1024;   // four resident blocks on each of 256 CUs

// S and the slice length (a multiple of 16 elements) of E elements: E alone decides them.
void opgrad_slices(int64_t E, int64_t* slices, int64_t* slice_len) {
    const int64_t S = E <= 0 ? 0 : std::min(kOgMaxSlices, ceil_div(E, kOgMinSlice));
    *slices = S;
    *slice_len = S ? ceil_div(ceil_div(E, S), (int64_t)fe::kOgChunk) * fe::kOgChunk : 0;
}

size_t opgrad_ws_bytes(int64_t slices, int64_t n_out) {
    return ((size_t)slices * (size_t)n_out * sizeof(double) + kReduceWsAlign - 1) / kReduceWsAlign * kReduceWsAlign;
}

// the three output strides must lay [n0][n1][n2] out as a dense array in some axis order (axes of extent 1: any stride)
bool opgrad_dense_layout(const int64_t (&st)[3], const int (&ext)[3]) {
    int order[3] = {0, 1, 2};
    std::sort(order, order + 3, [&](int x, int y) { return st[x] < st[y]; });
    int64_t expect = 1;
    for (int k : order) {
        if (ext[k] == 1) continue;
        if (st[k] != expect) return false;
        expect *= ext[k];
    }
    return true;
}

int opgrad_check_workspace(const char* what, const void* workspace, size_t workspace_bytes, size_t need) {
    if (need == 0) return FE_OK;
    if (!workspace) return fail(FE_EINVAL, "%s: null workspace (fe_opgrad_plan: %zu bytes)", what, need);
    if (workspace_bytes < need) return fail(FE_EINVAL, "%s: workspace of %zu bytes, the plan needs %zu", what, workspace_bytes, need);
    if (reinterpret_cast<uintptr_t>(workspace) % kReduceWsAlign)
        return fail(FE_EINVAL, "%s: workspace not %zu-byte aligned", what, kReduceWsAlign);
    return FE_OK;
}

template <int NM, int NN, bool FACE>
int launch_opgrad_partial(const fe::OpGradArgs& g, int64_t slices, hipStream_t s) {
    using G = fe::OpGradGeom<NM, NN, FACE>;
    const int lds = G::LDS_DOUBLES * (int)sizeof(double);
    static PerDeviceOnce once;
    if (int rc = configured(once, fe::opgrad_partial_kernel<NM, NN, FACE>, FACE ? "opgrad partials (face-mass)" : "opgrad partials",
                            lds, fe::kOgThreads, 4))
        return rc;
    hipLaunchKernelGGL((fe::opgrad_partial_kernel<NM, NN, FACE>), dim3((unsigned)slices), dim3(fe::kOgThreads), lds, s, g);
    FE_HIP_CHECK(hipGetLastError());
    return FE_OK;
}

// the partial launches of all fields (kOgMaxFields per launch, the later ones adding to their slices), then the combine
template <typename Launch>
int opgrad_run(fe::OpGradArgs& g, const double* const* a, const double* const* b, int nb_all, double* out, int64_t slices,
               hipStream_t s, Launch&& launch) {
    for (int k0 = 0; k0 < nb_all && slices > 0; k0 += fe::kOgMaxFields) {
        g.nb = std::min(nb_all - k0, fe::kOgMaxFields);
        for (int k = 0; k < fe::kOgMaxFields; ++k) {
            g.a[k] = k < g.nb ? a[k0 + k] : nullptr;
            g.b[k] = k < g.nb ? b[k0 + k] : nullptr;
        }
        g.accumulate = k0 > 0 ? 1 : 0;
        if (int rc = launch(g)) return rc;
    }
    if (int rc = launch_reduce_combine<double>("reduce combine f64", g.ws, out, g.n_out, slices, s)) return rc;
    FE_HIP_CHECK(hipGetLastError());
    return FE_OK;
}

}  // namespace

extern "C" {

int fe_opgrad_plan(int64_t E, int32_t n_out_entries, int64_t* slices, size_t* workspace_bytes) {
    if (E < 0) return fail(FE_EINVAL, "opgrad plan: E must be >= 0 (got %lld)", (long long)E);
    if (n_out_entries < 1) return fail(FE_EINVAL, "opgrad plan: %d output entries", n_out_entries);
    if (!slices || !workspace_bytes) return fail(FE_EINVAL, "opgrad plan: null pointer");
    int64_t len;
    opgrad_slices(E, slices, &len);
    *workspace_bytes = opgrad_ws_bytes(*slices, n_out_entries);
    return FE_OK;
}

int fe_opgrad_f64(const double* J, const double* const* a, const double* const* b, double* out, int64_t E, int32_t nb,
                  int32_t X, int32_t R, int32_t Np, int64_t jx, int64_t jr, int64_t je, int64_t sr, int64_t sp,
                  int64_t sq, void* workspace, size_t workspace_bytes, void* stream) {
    if (E < 0) return fail(FE_EINVAL, "opgrad: E must be >= 0 (got %lld)", (long long)E);
    if (nb < 1) return fail(FE_EINVAL, "opgrad: nb=%d, need at least one field", nb);
    if (X < 1 || X > 3 || R < 1 || R > 3) return fail(FE_EUNSUPPORTED, "opgrad: X = %d, R = %d not compiled (1..3)", X, R);
    switch (Np) {
        case 3: case 4: case 6: case 10: case 15: case 20: case 21: case 35: break;
        default: return fail(FE_EUNSUPPORTED, "opgrad: Np = %d not compiled (3, 4, 6, 10, 15, 20, 21, 35)", Np);
    }
    if (!a || !b || !out || (E > 0 && !J)) return fail(FE_EINVAL, "opgrad: null pointer");
    if (!aligned8(J) || !aligned8(out)) return fail(FE_EINVAL, "opgrad: device pointers must be 8-byte aligned (float64 arrays)");
    for (int k = 0; k < nb; ++k) {
        if (E > 0 && (!a[k] || !b[k])) return fail(FE_EINVAL, "opgrad: null device pointer (field %d)", k);
        if (!aligned8(a[k]) || !aligned8(b[k])) return fail(FE_EINVAL, "opgrad: device pointers must be 8-byte aligned (float64 arrays)");
    }
    if (jx < 0 || jr < 0 || je < 0) return fail(FE_EINVAL, "opgrad: negative J stride");
    const int64_t st[3] = {sr, sp, sq};
    const int ext[3] = {R, Np, Np};
    if (!opgrad_dense_layout(st, ext))
        return fail(FE_EINVAL, "opgrad: output strides (%lld, %lld, %lld) are no dense layout of [%d][%d][%d]", (long long)sr,
                    (long long)sp, (long long)sq, R, Np, Np);
    if (E * (int64_t)Np * X >= (int64_t)1 << 39) return fail(FE_EINVAL, "opgrad: E too large");
    int64_t slices, slice_len;
    opgrad_slices(E, &slices, &slice_len);
    const int64_t n_out = (int64_t)R * Np * Np;
    if (int rc = opgrad_check_workspace("opgrad", workspace, workspace_bytes, opgrad_ws_bytes(slices, n_out))) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    fe::OpGradArgs g = {};
    g.J = J, g.ws = static_cast<double*>(workspace);
    g.E = E, g.slice_len = slice_len, g.n_out = n_out;
    g.jx = jx, g.jr = jr, g.je = je, g.sr = sr, g.sp = sp, g.sq = sq;
    g.X = X, g.R = R;
    return opgrad_run(g, a, b, nb, out, slices, s, [&](const fe::OpGradArgs& ga) {
        switch (Np) {
            case 3: return launch_opgrad_partial<3, 3, false>(ga, slices, s);
            case 4: return launch_opgrad_partial<4, 4, false>(ga, slices, s);
            case 6: return launch_opgrad_partial<6, 6, false>(ga, slices, s);
            case 10: return launch_opgrad_partial<10, 10, false>(ga, slices, s);
            case 15: return launch_opgrad_partial<15, 15, false>(ga, slices, s);
            case 20: return launch_opgrad_partial<20, 20, false>(ga, slices, s);
            case 21: return launch_opgrad_partial<21, 21, false>(ga, slices, s);
            default: return launch_opgrad_partial<35, 35, false>(ga, slices, s);
        }
    });
}

int fe_facemass_opgrad_f64(const double* J, const double* const* g, const double* const* v, double* dR, int64_t E,
                           int32_t Np, int32_t nf, int32_t Nfp, int32_t b, int32_t layout_flags, void* workspace,
                           size_t workspace_bytes, void* stream) {
    if (E < 0) return fail(FE_EINVAL, "facemass opgrad: E must be >= 0 (got %lld)", (long long)E);
    if (b < 1) return fail(FE_EINVAL, "facemass opgrad: b=%d, need at least one field", b);
    if (layout_flags & ~(FE_FM_J_FE | FE_FM_R_IFJ | FE_FM_R_T))
        return fail(FE_EINVAL, "facemass opgrad: bad layout flags %d", layout_flags);
    int kind = -1;   // compiled shapes
    if (nf == 4 && Np == 4 && Nfp == 3) kind = 0;
    else if (nf == 4 && Np == 10 && Nfp == 6) kind = 1;
    else if (nf == 4 && Np == 20 && Nfp == 10) kind = 2;
    else if (nf == 4 && Np == 35 && Nfp == 15) kind = 3;
    else if (nf == 3 && Np == 3 && Nfp == 2) kind = 4;
    else if (nf == 3 && Np == 6 && Nfp == 3) kind = 5;
    else if (nf == 3 && Np == 10 && Nfp == 4) kind = 6;
    else if (nf == 3 && Np == 15 && Nfp == 5) kind = 7;
    else if (nf == 3 && Np == 21 && Nfp == 6) kind = 8;
    if (kind < 0)
        return fail(FE_EUNSUPPORTED, "facemass opgrad: (nf, Np, Nfp) = (%d, %d, %d) not compiled", nf, Np, Nfp);
    if (!g || !v || !dR || (E > 0 && !J)) return fail(FE_EINVAL, "facemass opgrad: null pointer");
    if (!aligned8(J) || !aligned8(dR)) return fail(FE_EINVAL, "facemass opgrad: device pointers must be 8-byte aligned");
    for (int k = 0; k < b; ++k) {
        if (E > 0 && (!g[k] || !v[k])) return fail(FE_EINVAL, "facemass opgrad: null device pointer (field %d)", k);
        if (!aligned8(g[k]) || !aligned8(v[k])) return fail(FE_EINVAL, "facemass opgrad: device pointers must be 8-byte aligned");
    }
    if (E * (int64_t)Np * b >= (int64_t)1 << 39) return fail(FE_EINVAL, "facemass opgrad: E too large");
    int64_t slices, slice_len;
    opgrad_slices(E, &slices, &slice_len);
    const int64_t n_out = (int64_t)nf * Np * Nfp;
    if (int rc = opgrad_check_workspace("facemass opgrad", workspace, workspace_bytes, opgrad_ws_bytes(slices, n_out))) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // dR's strides of (f, i, j): 'fij', 'ifj', 'fji', 'jfi' (as the face-mass kernels read R)
    const int rl = ((layout_flags & FE_FM_R_IFJ) ? 1 : 0) | ((layout_flags & FE_FM_R_T) ? 2 : 0);
    const int sF = rl == 0 ? Np * Nfp : rl == 1 ? Nfp : rl == 2 ? Nfp * Np : Np;
    const int sI = rl == 0 ? Nfp : rl == 1 ? nf * Nfp : 1;
    const int sJ = rl == 0 || rl == 1 ? 1 : rl == 2 ? Np : nf * Np;
    const bool jfe = (layout_flags & FE_FM_J_FE) != 0;
    fe::OpGradArgs a = {};
    a.J = J, a.ws = static_cast<double*>(workspace);
    a.E = E, a.slice_len = slice_len, a.n_out = n_out;
    a.jx = 0, a.jr = jfe ? E : 1, a.je = jfe ? 1 : nf;
    a.sr = sF, a.sp = sJ, a.sq = sI;   // rows of the tiles are j (the planes of v), columns i (g)
    a.X = 1, a.R = nf;
    return opgrad_run(a, g, v, b, dR, slices, s, [&](const fe::OpGradArgs& ga) {
        switch (kind) {
            case 0: return launch_opgrad_partial<3, 4, true>(ga, slices, s);
            case 1: return launch_opgrad_partial<6, 10, true>(ga, slices, s);
            case 2: return launch_opgrad_partial<10, 20, true>(ga, slices, s);
            case 3: return launch_opgrad_partial<15, 35, true>(ga, slices, s);
            case 4: return launch_opgrad_partial<2, 3, true>(ga, slices, s);
            case 5: return launch_opgrad_partial<3, 6, true>(ga, slices, s);
            case 6: return launch_opgrad_partial<4, 10, true>(ga, slices, s);
            case 7: return launch_opgrad_partial<5, 15, true>(ga, slices, s);
            default: return launch_opgrad_partial<6, 21, true>(ga, slices, s);
        }
    });
}

}  // extern "C"

// ---- element-local operator of any shape (fe_elemop.h) ----
namespace {

constexpr int kKindElementOperator = 1024;   // fe_last_launch_info `kind`

// the largest dynamic LDS of the shapes that run on elemop_kernel<RT>: what the residency of the instantiation is checked at
int elemop_lds_max(int rt) {
    int most = 0;
    for (int ni = 16 * rt - 15; ni <= 16 * rt; ++ni)
        for (int nj = 1; nj <= fe::kElemOpMaxN; ++nj)
            if (fe::elemop_supported(ni, nj)) most = std::max(most, fe::elemop_lds_bytes(ni, nj));
    return most;
}

template <int RT>
int launch_elemop(const fe::ElemOpArgs& g, hipStream_t s) {
    static const std::string what = "element operator RT=" + std::to_string(RT);
    if (int rc = configured<fe::elemop_kernel<RT>>(what.c_str(), elemop_lds_max(RT), fe::kElemOpThreads, 2)) return rc;
    const unsigned grid = persistent_grid(g.n_tiles * g.nb, fe::kElemOpWaves);
    hipLaunchKernelGGL(fe::elemop_kernel<RT>, dim3(grid), dim3(fe::kElemOpThreads), fe::elemop_lds_bytes(g.Ni, g.Nj), s, g);
    FE_HIP_CHECK(hipGetLastError());
    note_launch(false, 0, grid, fe::kElemOpWaves, g.n_tiles, g.n_tiles, kKindElementOperator);
    return FE_OK;
}

}  // namespace

extern "C" {

int fe_elemop_supported(int32_t Ni, int32_t Nj) { return fe::elemop_supported(Ni, Nj) ? 1 : 0; }

int fe_elemop_f64(const double* J, const double* A, const double* const* u, double* const* out, int64_t E, int32_t Ni,
                  int32_t Nj, int32_t b, int32_t op_flags, void* stream) {
    forget_last_launch();
    const bool sized = Ni > 0 && Nj > 0;
    // (J is optional: where it is null the operator stands in for it in the check of pointers)
    CallCheck c = {"elemop", J ? static_cast<const void*>(J) : A, A, ptr_table(u), ptr_table(out), E,
                   sized ? std::max(Ni, Nj) : std::min(Ni, Nj), b, op_flags, FE_OP_TRANSPOSED};
    FE_CHECK_CALL(c);
    if (!fe::elemop_supported(Ni, Nj))
        return fail(FE_EUNSUPPORTED, "elemop: (Ni, Nj) = (%d, %d) is outside the size rule (1 <= Ni, Nj <= %d and "
                    "ceil(Ni / 16) * ceil(Nj / 4) <= %d)", Ni, Nj, fe::kElemOpMaxN, fe::kElemOpMaxFragments);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t n_tiles = (E + 15) / 16;
    for (int k0 = 0; k0 < b; k0 += fe::kMaxFields) {     // at most kMaxFields fields per launch
        fe::ElemOpArgs g = {};
        g.J = J, g.A = A, g.E = E, g.n_tiles = n_tiles;
        g.Ni = Ni, g.Nj = Nj, g.KS = fe::elemop_k_steps(Nj), g.nb = std::min(b - k0, fe::kMaxFields);
        g.opT = (op_flags & FE_OP_TRANSPOSED) ? 1 : 0;
        g.buf_doubles = fe::elemop_buffer_doubles(Ni, Nj);
        g.magic_ni = (unsigned)(((1u << 20) + Ni - 1) / Ni);
        for (int k = 0; k < g.nb; ++k) g.f.v[k] = u[k0 + k], g.f.out[k] = out[k0 + k];
        int rc;
        switch (fe::elemop_row_tiles(Ni)) {
            case 1: rc = launch_elemop<1>(g, s); break;
            case 2: rc = launch_elemop<2>(g, s); break;
            case 3: rc = launch_elemop<3>(g, s); break;
            case 4: rc = launch_elemop<4>(g, s); break;
            case 5: rc = launch_elemop<5>(g, s); break;
            default: rc = launch_elemop<6>(g, s); break;
        }
        if (rc != FE_OK) return rc;
    }
    return FE_OK;
}

}  // extern "C"

// ---- weighted element operator iq,eq,qj,ej->ei (fe_weightedop.h) ----
namespace {

constexpr int kKindWeightedElementOperator = 2048;   // fe_last_launch_info `kind`

// the largest dynamic LDS of the shapes that run on weightedop_kernel<RQ, RI>: what the residency of the instantiation is checked at
int weightedop_lds_max(int rq, int ri) {
    int most = 0;
    for (int ni = 16 * ri - 15; ni <= 16 * ri; ++ni)
        for (int nq = 16 * rq - 15; nq <= 16 * rq; ++nq)
            for (int nj = 1; nj <= fe::kWtOpMaxN; ++nj)
                if (fe::weightedop_supported(ni, nq, nj)) most = std::max(most, fe::weightedop_lds_bytes(ni, nq, nj));
    return most;
}

template <int RQ, int RI>
int launch_weightedop(const fe::WtOpArgs& g, hipStream_t s) {
    static const std::string what = "weighted element operator RQ=" + std::to_string(RQ) + " RI=" + std::to_string(RI);
    static const int lds_max = weightedop_lds_max(RQ, RI);
    if (int rc = configured<fe::weightedop_kernel<RQ, RI>>(what.c_str(), lds_max, fe::kWtOpThreads, 2)) return rc;
    const unsigned grid = persistent_grid(g.n_tiles, fe::kWtOpWaves);
    hipLaunchKernelGGL((fe::weightedop_kernel<RQ, RI>), dim3(grid), dim3(fe::kWtOpThreads),
                       fe::weightedop_lds_bytes(g.Ni, g.Nq, g.Nj), s, g);
    FE_HIP_CHECK(hipGetLastError());
    note_launch(false, 0, grid, fe::kWtOpWaves, g.n_tiles, g.n_tiles, kKindWeightedElementOperator);
    return FE_OK;
}

template <int RQ>
int launch_weightedop_rq(int ri, const fe::WtOpArgs& g, hipStream_t s) {
    switch (ri) {
        case 1: return launch_weightedop<RQ, 1>(g, s);
        case 2: return launch_weightedop<RQ, 2>(g, s);
        default: return launch_weightedop<RQ, 3>(g, s);
    }
}

}  // namespace

extern "C" {

int fe_weightedop_supported(int32_t Ni, int32_t Nq, int32_t Nj) { return fe::weightedop_supported(Ni, Nq, Nj) ? 1 : 0; }

int fe_weightedop_f64(const double* P, const double* W, const double* A, const double* const* u, double* const* out, int64_t E,
                      int32_t Ni, int32_t Nq, int32_t Nj, int32_t b, int32_t op_flags, void* stream) {
    forget_last_launch();
    const bool sized = Ni > 0 && Nq > 0 && Nj > 0;
    CallCheck c = {"weightedop", W, A, ptr_table(u), ptr_table(out), E,
                   sized ? std::max(Ni, std::max(Nq, Nj)) : std::min(Ni, std::min(Nq, Nj)), b, op_flags, FE_WO_P_T | FE_WO_A_T};
    c.op2 = P, c.has_op2 = true;
    FE_CHECK_CALL(c);
    if (!fe::weightedop_supported(Ni, Nq, Nj))
        return fail(FE_EUNSUPPORTED, "weightedop: (Ni, Nq, Nj) = (%d, %d, %d) is outside the size rule (1 <= Ni, Nj <= %d, 1 <= Nq <= %d "
                    "and both operator images with four wave buffers within %d bytes of LDS)", Ni, Nq, Nj, fe::kWtOpMaxN,
                    fe::kWtOpMaxQ, fe::kWtOpMaxLds);
    hipStream_t s = static_cast<hipStream_t>(stream);
    for (int k0 = 0; k0 < b; k0 += fe::kMaxFields) {     // at most kMaxFields fields per launch
        fe::WtOpArgs g = {};
        g.P = P, g.W = W, g.A = A, g.E = E, g.n_tiles = (E + 15) / 16;
        g.Ni = Ni, g.Nq = Nq, g.Nj = Nj, g.KJ = fe::elemop_k_steps(Nj), g.KQ = fe::elemop_k_steps(Nq);
        g.nb = std::min(b - k0, fe::kMaxFields);
        g.pT = (op_flags & FE_WO_P_T) ? 1 : 0, g.aT = (op_flags & FE_WO_A_T) ? 1 : 0;
        g.buf_doubles = fe::weightedop_buffer_doubles(Ni, Nq, Nj);
        g.magic_ni = (unsigned)(((1u << 20) + Ni - 1) / Ni);
        for (int k = 0; k < g.nb; ++k) g.f.v[k] = u[k0 + k], g.f.out[k] = out[k0 + k];
        int rc;
        switch (fe::elemop_row_tiles(Nq)) {
            case 1: rc = launch_weightedop_rq<1>(fe::elemop_row_tiles(Ni), g, s); break;
            case 2: rc = launch_weightedop_rq<2>(fe::elemop_row_tiles(Ni), g, s); break;
            case 3: rc = launch_weightedop_rq<3>(fe::elemop_row_tiles(Ni), g, s); break;
            default: rc = launch_weightedop_rq<4>(fe::elemop_row_tiles(Ni), g, s); break;
        }
        if (rc != FE_OK) return rc;
    }
    return FE_OK;
}

}  // extern "C"

// ---- weight gradient of the weighted element operator, iq,qj,ej,ei->eq (fe_weightgrad.h) ----
namespace {

constexpr int kKindWeightedWeightAdjoint = 4096;   // fe_last_launch_info `kind`

// the largest dynamic LDS of the shapes that run on wgrad_kernel<RQ>: what the residency of the instantiation is checked at
int weightgrad_lds_max(int rq) {
    int most = 0;
    for (int ni = 1; ni <= fe::kWGradMaxN; ++ni)
        for (int nq = 16 * rq - 15; nq <= 16 * rq; ++nq)
            for (int nj = 1; nj <= fe::kWGradMaxN; ++nj)
                if (fe::weightgrad_supported(ni, nq, nj)) most = std::max(most, fe::weightgrad_lds_bytes(ni, nq, nj));
    return most;
}

template <int RQ>
int launch_weightgrad(const fe::WGradArgs& g, hipStream_t s) {
    static const std::string what = "weight gradient RQ=" + std::to_string(RQ);
    static const int lds_max = weightgrad_lds_max(RQ);
    if (int rc = configured<fe::wgrad_kernel<RQ>>(what.c_str(), lds_max, fe::kWGradThreads, 2)) return rc;
    const unsigned grid = persistent_grid(g.n_tiles, fe::kWGradWaves);
    hipLaunchKernelGGL(fe::wgrad_kernel<RQ>, dim3(grid), dim3(fe::kWGradThreads), fe::weightgrad_lds_bytes(g.Ni, g.Nq, g.Nj), s, g);
    FE_HIP_CHECK(hipGetLastError());
    note_launch(false, 0, grid, fe::kWGradWaves, g.n_tiles, g.n_tiles, kKindWeightedWeightAdjoint);
    return FE_OK;
}

}  // namespace

extern "C" {

int fe_weightgrad_supported(int32_t Ni, int32_t Nq, int32_t Nj) { return fe::weightgrad_supported(Ni, Nq, Nj) ? 1 : 0; }

int fe_weightgrad_f64(const double* P, const double* A, const double* const* u, const double* const* g, double* dW, int64_t E,
                      int32_t Ni, int32_t Nq, int32_t Nj, int32_t b, int32_t op_flags, void* stream) {
    forget_last_launch();
    const bool sized = Ni > 0 && Nq > 0 && Nj > 0;
    // (the check of fe_weightedop_f64, its order and its texts: dW stands where W does, the g_k where the outputs do)
    CallCheck c = {"weightgrad", dW, A, ptr_table(u), ptr_table(g), E,
                   sized ? std::max(Ni, std::max(Nq, Nj)) : std::min(Ni, std::min(Nq, Nj)), b, op_flags, FE_WO_P_T | FE_WO_A_T};
    c.op2 = P, c.has_op2 = true;
    if (b > fe::kMaxFields && E >= 0 && sized)
        return fail(FE_EINVAL, "weightgrad: b=%d, need at least one field and at most %d (the rows are summed in one launch)", b,
                    fe::kMaxFields);
    FE_CHECK_CALL(c);
    if (!fe::weightgrad_supported(Ni, Nq, Nj))
        return fail(FE_EUNSUPPORTED, "weightgrad: (Ni, Nq, Nj) = (%d, %d, %d) is outside the size rule (1 <= Ni, Nj <= %d, 1 <= Nq <= %d "
                    "and both operator images with four wave buffers within %d bytes of LDS)", Ni, Nq, Nj, fe::kWGradMaxN,
                    fe::kWGradMaxQ, fe::kWGradMaxLds);
    fe::WGradArgs a = {};
    a.P = P, a.A = A, a.dW = dW, a.E = E, a.n_tiles = (E + 15) / 16;
    a.Ni = Ni, a.Nq = Nq, a.Nj = Nj, a.KI = fe::elemop_k_steps(Ni), a.KJ = fe::elemop_k_steps(Nj), a.nb = b;
    a.pT = (op_flags & FE_WO_P_T) ? 1 : 0, a.aT = (op_flags & FE_WO_A_T) ? 1 : 0;
    a.buf_doubles = fe::weightgrad_buffer_doubles(Ni, Nq, Nj);
    a.magic_nq = (unsigned)(((1u << 20) + Nq - 1) / Nq);
    for (int k = 0; k < b; ++k) a.item[2 * k] = u[k], a.item[2 * k + 1] = g[k];
    for (int k = 2 * b; k < 2 * fe::kMaxFields; ++k) a.item[k] = u[0];
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (fe::elemop_row_tiles(Nq)) {
        case 1: return launch_weightgrad<1>(a, s);
        case 2: return launch_weightgrad<2>(a, s);
        case 3: return launch_weightgrad<3>(a, s);
        default: return launch_weightgrad<4>(a, s);
    }
}

}  // extern "C"
