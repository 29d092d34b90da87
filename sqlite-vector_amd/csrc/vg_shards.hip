// vg_shards.hip - one logical corpus spread over several devices of ONE process (the SQLite extension's case: a
// connection lives in one process).  Host code only: every distance is computed by the per-device
// corpora of vg_api.hip; this file distributes rows, puts all shards in flight and merges their candidate keys.
//
// Distribution is block-cyclic in scan order: global position g lives in block b = g / B, on shard b % S, at local
// position (b / S) * B + g % B.  Local order is therefore monotone in global order, so each shard's own
// (distance, local position) ranking is consistent with the global (distance, scan position) contract and the
// merge only has to compare (distance image, global position) - the result is bit-identical to one big shard.
// Rows can be appended as they stream out of sqlite3_step() without knowing the final count (a contiguous
// row-range split would need it), and every device gets work as soon as B * S rows exist.
//
// The exchange step - S x 64 candidate keys, 512 B per shard - has two forms, chosen per handle (vg_shards_set_gather, the
// VECTORGPU_SHARD_GATHER environment variable: host | rccl):
//   host  (default) every shard copies its 64 keys to pinned host memory behind its scan, one host thread waits for the S streams;
//   rccl            north_star's "RCCL gather of per-shard candidates over xGMI": one communicator per device of this process
//                   (ncclCommInitAll), ONE grouped ncclAllGather of 64 keys per shard on the scan streams, then a single 512 B x S
//                   copy from the first device.  librccl.so is dlopen'ed on first use (the library has no link-time dependency
//                   on it); the devices of a handle must be distinct (RCCL refuses two ranks on one device) - otherwise, or if
//                   the library / a call fails, the handle stays with the host gather.
// Both produce the same S x 64 keys, so the merge - and the result - is identical bit for bit; which one is faster is a
// measurement (tools/shards_gather_bench.py): the payload is latency-bound either way.  The one-process-per-GPU variant of the
// same exchange (torch.distributed / RCCL) is shard.py.
#include "vg_internal.h"
#include "vg_refslots.h"

#include <dlfcn.h>

#include <algorithm>
#include <cstdio>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

extern "C" void vg_set_last_error_(const char *msg);          // vg_api.hip (thread-local error slot)

#define VG_WAVE_KEYS 64

struct vg_shards {
    int S = 0;
    int64_t B = 0;
    int vtype = 0, dim = 0, es = 0;
    int64_t n_rows = 0;
    int64_t rowid_base = 1;
    int tie_order = VG_TIE_POSITION;
    std::vector<vg_corpus *> sh;
    std::vector<int> devices;
    // ---- the RCCL form of the candidate gather (see the file header)
    int gather_mode = 0;                       // 0 = host, 1 = rccl
    std::vector<void *> comms;                 // ncclComm_t per shard (empty until first use)
    std::vector<uint64_t *> d_gather;          // per shard: S x 64 keys (the all-gather's receive buffer)
    uint64_t *h_gather = nullptr;              // pinned: S x 64 keys
    bool rccl_failed = false;
    unsigned long long gather_calls[2] = {0, 0};
    // tie_order = reference (see shards_scan_topk_fused): the same counters and the same "ties were seen recently" rule as one corpus'
    int ref_hot = 0;
    unsigned long long ref_stats[4] = {0, 0, 0, 0};   // reference-order scans | with a tie among the k+1 best | fused replays | store-mode replays
    struct ShardPool *pool = nullptr;          // persistent host threads, one per shard behind the first (see pool_run)
    // the last vg_shards_scan_within (S > 1): the shards' matches merged by (distance image, GLOBAL position), kept for the fetch
    struct WithinHit { uint64_t key; int64_t gpos; int shard; };   // key: the shard's own (image << 32 | local position)
    std::vector<WithinHit> within_hits;
    std::vector<std::vector<WithinHit>> within_batch_hits;   // the last vg_shards_scan_within_batch (S > 1): the same, per query
    int threaded = 0;                          // per-query issue + collect of the shards on those threads
};

// ---- librccl.so, resolved at run time
namespace {
typedef int (*nccl_comm_init_all_t)(void **, int, const int *);
typedef int (*nccl_all_gather_t)(const void *, void *, size_t, int, void *, hipStream_t);
typedef int (*nccl_group_t)(void);
typedef int (*nccl_comm_destroy_t)(void *);
typedef const char *(*nccl_error_string_t)(int);
struct RcclApi {
    void *lib = nullptr;
    nccl_comm_init_all_t comm_init_all = nullptr;
    nccl_all_gather_t all_gather = nullptr;
    nccl_group_t group_start = nullptr, group_end = nullptr;
    nccl_comm_destroy_t comm_destroy = nullptr;
    nccl_error_string_t error_string = nullptr;
    bool tried = false;
};
RcclApi g_rccl;
const int kNcclUint64 = 5;                      // ncclUint64 (rccl.h ncclDataType_t)
bool rccl_load() {
    if (g_rccl.tried) return g_rccl.lib != nullptr;
    g_rccl.tried = true;
    const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char *n : names) if ((g_rccl.lib = dlopen(n, RTLD_NOW | RTLD_LOCAL))) break;
    if (!g_rccl.lib) return false;
    g_rccl.comm_init_all = (nccl_comm_init_all_t)dlsym(g_rccl.lib, "ncclCommInitAll");
    g_rccl.all_gather = (nccl_all_gather_t)dlsym(g_rccl.lib, "ncclAllGather");
    g_rccl.group_start = (nccl_group_t)dlsym(g_rccl.lib, "ncclGroupStart");
    g_rccl.group_end = (nccl_group_t)dlsym(g_rccl.lib, "ncclGroupEnd");
    g_rccl.comm_destroy = (nccl_comm_destroy_t)dlsym(g_rccl.lib, "ncclCommDestroy");
    g_rccl.error_string = (nccl_error_string_t)dlsym(g_rccl.lib, "ncclGetErrorString");
    if (!g_rccl.comm_init_all || !g_rccl.all_gather || !g_rccl.group_start || !g_rccl.group_end || !g_rccl.comm_destroy) {
        dlclose(g_rccl.lib);
        g_rccl.lib = nullptr;
    }
    return g_rccl.lib != nullptr;
}
}

static int fail(int code, const char *msg) {
    vg_set_last_error_(msg);
    return code;
}
int vg_scan_topk_enqueue_dev(vg_corpus *c, int metric, const void *query, int k);    // vg_api.hip: keys stay in c->d_keys

static inline void locate(const vg_shards *s, int64_t g, int *shard, int64_t *local) {
    const int64_t b = g / s->B;
    *shard = (int)(b % s->S);
    *local = (b / s->S) * s->B + g % s->B;
}

static inline int64_t global_of(const vg_shards *s, int shard, int64_t local) {
    return ((local / s->B) * s->S + shard) * s->B + local % s->B;
}

// ---- PERSISTENT host threads for the per-query work (one thread issued S x (hipSetDevice + H2D + launches) and then collected
// S times - on eight real devices ~0.1 ms of a 2.4 ms scan of a 12.5M-row shard).  Shard i >= 1 has a thread of its own, bound to the
// shard's device once; a query wakes them all, the calling thread serves shard 0 itself, and every thread enqueues AND collects its
// shard.  On by default when the shards sit on more than one device; VECTORGPU_SHARD_THREADS=1 / 0 forces it (the tests run it over
// logical shards of one device).
struct ShardPool {
    std::vector<std::thread> th;
    std::mutex mu;
    std::condition_variable go, done;
    uint64_t epoch = 0;
    int pending = 0;
    bool quit = false;
    std::function<int(int)> job;
    std::vector<int> rc;
    std::vector<std::string> msg;
};
static void pool_worker(vg_shards *s, ShardPool *p, int shard) {
    hipSetDevice(s->devices[(size_t)shard]);
    uint64_t seen = 0;
    for (;;) {
        std::unique_lock<std::mutex> lk(p->mu);
        p->go.wait(lk, [&] { return p->quit || p->epoch != seen; });
        if (p->quit) return;
        seen = p->epoch;
        lk.unlock();
        const int r = p->job(shard);
        const std::string m = r != VG_OK ? vg_last_error() : "";
        lk.lock();
        p->rc[(size_t)shard] = r;
        if (r != VG_OK) p->msg[(size_t)shard] = m;
        if (--p->pending == 0) p->done.notify_one();
    }
}
static void pool_release(vg_shards *s) {
    ShardPool *p = s->pool;
    if (!p) return;
    { std::lock_guard<std::mutex> lk(p->mu); p->quit = true; }
    p->go.notify_all();
    for (auto &t : p->th) t.join();
    delete p;
    s->pool = nullptr;
}
// fn(shard) for every shard at once; the first failure's code and message are re-raised on the calling thread
template <typename F>
static int pool_run(vg_shards *s, F fn) {
    if (s->S == 1) return fn(0);
    if (!s->pool) {
        s->pool = new ShardPool();
        s->pool->rc.assign((size_t)s->S, VG_OK);
        s->pool->msg.assign((size_t)s->S, std::string());
        for (int i = 1; i < s->S; ++i) s->pool->th.emplace_back(pool_worker, s, s->pool, i);
    }
    ShardPool *p = s->pool;
    {
        std::lock_guard<std::mutex> lk(p->mu);
        p->job = fn;
        p->pending = s->S - 1;
        std::fill(p->rc.begin(), p->rc.end(), VG_OK);
        ++p->epoch;
    }
    p->go.notify_all();
    const int r0 = fn(0);
    const std::string m0 = r0 != VG_OK ? vg_last_error() : "";
    {
        std::unique_lock<std::mutex> lk(p->mu);
        p->done.wait(lk, [&] { return p->pending == 0; });
    }
    if (r0 != VG_OK) return fail(r0, m0.c_str());
    for (int i = 1; i < s->S; ++i)
        if (p->rc[(size_t)i] != VG_OK) return fail(p->rc[(size_t)i], p->msg[(size_t)i].c_str());
    return VG_OK;
}

// run fn(shard) for every shard concurrently (one host thread each: the per-corpus calls block on their stream);
// the first failure's code and message are re-raised on the calling thread
template <typename F>
static int for_each_shard(vg_shards *s, F fn) {
    if (s->S == 1) return fn(0);
    std::vector<int> rc((size_t)s->S, VG_OK);
    std::vector<std::string> msg((size_t)s->S);
    std::vector<std::thread> th;
    for (int i = 0; i < s->S; ++i)
        th.emplace_back([&, i] {
            rc[(size_t)i] = fn(i);
            if (rc[(size_t)i] != VG_OK) msg[(size_t)i] = vg_last_error();
        });
    for (auto &t : th) t.join();
    for (int i = 0; i < s->S; ++i)
        if (rc[(size_t)i] != VG_OK) return fail(rc[(size_t)i], msg[(size_t)i].c_str());
    return VG_OK;
}

extern "C" int vg_shards_create(const int *devices, int n_devices, int vtype, int dim, int64_t block_rows, vg_shards **out) {
    if (!out) return fail(VG_ERR_INVALID, "vg_shards_create: out is NULL");
    *out = nullptr;
    if (n_devices < 1 || n_devices > 64) return fail(VG_ERR_INVALID, "vg_shards_create: 1..64 shards");
    vg_shards *s = new vg_shards();
    s->S = n_devices;
    s->B = block_rows > 0 ? block_rows : 65536;
    s->vtype = vtype;
    s->dim = dim;
    {
        vg_switches_read();                                           // (a shard set, like a corpus, takes the environment as it is now)
        s->gather_mode = vg_sw(SW_VECTORGPU_SHARD_GATHER, 0);
    }
    for (int i = 0; i < n_devices; ++i) {
        vg_corpus *c = nullptr;
        s->devices.push_back(devices ? devices[i] : i);
        int rc = vg_corpus_create(devices ? devices[i] : i, vtype, dim, 0, &c);
        if (rc != VG_OK) {
            for (auto *p : s->sh) vg_corpus_destroy(p);
            delete s;
            return rc;
        }
        s->sh.push_back(c);
    }
    s->es = (vtype == VG_TYPE_F32) ? 4 : (vtype == VG_TYPE_F16 || vtype == VG_TYPE_BF16) ? 2 : 1;
    {
        bool many = false;
        for (int d : s->devices) many = many || d != s->devices[0];
        s->threaded = vg_sw(SW_VECTORGPU_SHARD_THREADS, many ? 1 : 0) != 0 && s->S > 1;
    }
    *out = s;
    return VG_OK;
}

static void rccl_release(vg_shards *s) {
    for (size_t i = 0; i < s->comms.size(); ++i) if (s->comms[i] && g_rccl.comm_destroy) g_rccl.comm_destroy(s->comms[i]);
    s->comms.clear();
    for (size_t i = 0; i < s->d_gather.size(); ++i)
        if (s->d_gather[i]) { hipSetDevice(s->devices[i]); hipFree(s->d_gather[i]); }
    s->d_gather.clear();
    if (s->h_gather) { hipHostFree(s->h_gather); s->h_gather = nullptr; }
}

extern "C" void vg_shards_destroy(vg_shards *s) {
    if (!s) return;
    pool_release(s);
    rccl_release(s);
    for (auto *p : s->sh) vg_corpus_destroy(p);
    delete s;
}

// communicators + receive buffers on first use; false (and the handle falls back to the host gather for good) when RCCL cannot
// serve this handle
static bool rccl_ready(vg_shards *s) {
    if (s->rccl_failed) return false;
    if (!s->comms.empty()) return true;
    bool distinct = true;
    for (int i = 0; i < s->S; ++i) for (int j = 0; j < i; ++j) distinct &= s->devices[(size_t)i] != s->devices[(size_t)j];
    if (!distinct || !rccl_load()) { s->rccl_failed = true; return false; }
    s->comms.assign((size_t)s->S, nullptr);
    if (g_rccl.comm_init_all(s->comms.data(), s->S, s->devices.data()) != 0) { s->comms.clear(); s->rccl_failed = true; return false; }
    s->d_gather.assign((size_t)s->S, nullptr);
    bool ok = true;
    for (int i = 0; i < s->S && ok; ++i) {
        ok = hipSetDevice(s->devices[(size_t)i]) == hipSuccess &&
             hipMalloc(&s->d_gather[(size_t)i], (size_t)s->S * VG_WAVE_KEYS * sizeof(uint64_t)) == hipSuccess;
    }
    ok = ok && hipHostMalloc(&s->h_gather, (size_t)s->S * VG_WAVE_KEYS * sizeof(uint64_t)) == hipSuccess;
    if (!ok) { (void)hipGetLastError(); rccl_release(s); s->rccl_failed = true; return false; }
    return true;
}

// The RCCL form of "scan every shard, bring the S x 64 candidate keys to the host": scans enqueued on the shards' streams with the
// keys left on their devices, one grouped all-gather on those streams, one copy from the first device.  VG_OK, or an error after
// which the caller repeats the query through the host gather.
static int rccl_scan_and_gather(vg_shards *s, int metric, const void *query, int kk, uint64_t *out_keys) {
    int rc = VG_OK;
    for (int i = 0; i < s->S && rc == VG_OK; ++i) rc = vg_scan_topk_enqueue_dev(s->sh[(size_t)i], metric, query, kk);
    if (rc != VG_OK) return rc;
    int nrc = g_rccl.group_start();
    for (int i = 0; i < s->S && nrc == 0; ++i) {
        vg_corpus *c = s->sh[(size_t)i];
        nrc = g_rccl.all_gather(c->d_keys, s->d_gather[(size_t)i], VG_WAVE_KEYS, kNcclUint64, s->comms[(size_t)i], c->stream);
    }
    const int erc = g_rccl.group_end();
    if (nrc != 0 || erc != 0) {
        for (int i = 0; i < s->S; ++i) { hipSetDevice(s->devices[(size_t)i]); hipStreamSynchronize(s->sh[(size_t)i]->stream); s->sh[(size_t)i]->enqueued = false; }
        return fail(VG_ERR_HIP, (g_rccl.error_string ? g_rccl.error_string(nrc ? nrc : erc) : "RCCL all-gather failed"));
    }
    vg_corpus *c0 = s->sh[0];
    HIP_TRY(hipSetDevice(s->devices[0]));
    HIP_TRY(hipMemcpyAsync(s->h_gather, s->d_gather[0], (size_t)s->S * VG_WAVE_KEYS * sizeof(uint64_t), hipMemcpyDeviceToHost, c0->stream));
    HIP_TRY(hipStreamSynchronize(c0->stream));                 // (every shard's keys arrived on device 0: all scans are done)
    for (int i = 0; i < s->S; ++i) {
        vg_corpus *c = s->sh[(size_t)i];
        c->enqueued = false;
        if (c->profiling && i > 0) {                           // its own all-gather kernel (and the events behind it) may still be running
            HIP_TRY(hipSetDevice(s->devices[(size_t)i]));
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
        vg_collect_timing(c);
    }
    memcpy(out_keys, s->h_gather, (size_t)s->S * VG_WAVE_KEYS * sizeof(uint64_t));
    ++s->gather_calls[1];
    return VG_OK;
}

extern "C" int vg_shards_set_gather(vg_shards *s, int mode) {
    if (!s) return fail(VG_ERR_INVALID, "shards handle is NULL");
    if (mode != 0 && mode != 1) return fail(VG_ERR_INVALID, "vg_shards_set_gather: 0 = host, 1 = rccl");
    s->gather_mode = mode;
    if (mode == 1 && s->rccl_failed) {                         // asked again explicitly: try again, with communicators of its own
        rccl_release(s);                                       // (the ones of a failed group call may be broken)
        s->rccl_failed = false;
    }
    return VG_OK;
}
// [0] queries answered through the host gather, [1] through the RCCL all-gather; returns the mode in effect (1 only when RCCL serves)
extern "C" int vg_shards_gather_stats(vg_shards *s, unsigned long long *out2) {
    if (!s) return 0;
    if (out2) { out2[0] = s->gather_calls[0]; out2[1] = s->gather_calls[1]; }
    return (s->gather_mode == 1 && !s->rccl_failed) ? 1 : 0;
}

extern "C" int vg_shards_clear(vg_shards *s) {
    if (!s) return fail(VG_ERR_INVALID, "shards handle is NULL");
    for (auto *p : s->sh) {
        int rc = vg_corpus_clear(p);
        if (rc != VG_OK) return rc;
    }
    s->n_rows = 0;
    return VG_OK;
}

extern "C" int vg_shards_count(const vg_shards *s) { return s ? s->S : 0; }
extern "C" int64_t vg_shards_rows(const vg_shards *s) { return s ? s->n_rows : 0; }
extern "C" vg_corpus *vg_shards_shard(const vg_shards *s, int i) { return (s && i >= 0 && i < s->S) ? s->sh[(size_t)i] : nullptr; }

extern "C" int vg_shards_reserve(vg_shards *s, int64_t total_rows) {
    if (!s) return fail(VG_ERR_INVALID, "shards handle is NULL");
    if (total_rows <= 0) return VG_OK;
    const int64_t blocks = (total_rows + s->B - 1) / s->B;
    for (int i = 0; i < s->S; ++i) {
        const int64_t mine = (blocks + s->S - 1 - i) / s->S;                   // blocks i, i+S, i+2S, ...
        if (mine <= 0) continue;
        const int64_t rows = std::min<int64_t>(mine * s->B, total_rows);
        int rc = vg_corpus_reserve(s->sh[(size_t)i], rows);
        if (rc != VG_OK) return rc;
    }
    return VG_OK;
}

extern "C" int vg_corpus_clone(const vg_corpus *src, vg_corpus **out);
extern "C" int vg_shards_clone(const vg_shards *src, vg_shards **out) {
    if (!src || !out) return fail(VG_ERR_INVALID, "vg_shards_clone: NULL argument");
    *out = nullptr;
    vg_shards *s = nullptr;
    int rc = vg_shards_create(src->devices.data(), src->S, src->vtype, src->dim, src->B, &s);
    if (rc != VG_OK) return rc;
    for (int i = 0; i < src->S; ++i) {
        vg_corpus *c = nullptr;
        rc = vg_corpus_clone(src->sh[(size_t)i], &c);
        if (rc != VG_OK) { vg_shards_destroy(s); return rc; }
        vg_corpus_destroy(s->sh[(size_t)i]);                                  // (the empty corpus vg_shards_create made)
        s->sh[(size_t)i] = c;
    }
    s->n_rows = src->n_rows;
    s->rowid_base = src->rowid_base;
    s->tie_order = src->tie_order;
    s->gather_mode = src->gather_mode;
    *out = s;
    return VG_OK;
}

extern "C" int vg_corpus_trim(vg_corpus *c);
extern "C" int vg_shards_trim(vg_shards *s) {
    if (!s) return fail(VG_ERR_INVALID, "shards handle is NULL");
    for (int i = 0; i < s->S; ++i) {
        int rc = vg_corpus_trim(s->sh[(size_t)i]);
        if (rc != VG_OK) return rc;
    }
    return VG_OK;
}

extern "C" int vg_shards_set_rowid_base(vg_shards *s, int64_t base) {
    if (!s) return fail(VG_ERR_INVALID, "shards handle is NULL");
    s->rowid_base = base;
    if (s->S == 1) return vg_corpus_set_rowid_base(s->sh[0], base);
    return VG_OK;
}

// rows (or [rowid | vector] records when record_mode) are dealt out block by block
static int append_common(vg_shards *s, const void *host, int64_t n, int64_t stride, const int64_t *rowids, bool record_mode) {
    if (!s) return fail(VG_ERR_INVALID, "shards handle is NULL");
    if (n == 0) return VG_OK;
    if (!host || n < 0) return fail(VG_ERR_INVALID, "vg_shards_append: bad rows pointer / count");
    const uint8_t *p = (const uint8_t *)host;
    std::vector<int64_t> gen;
    int64_t done = 0;
    while (done < n) {
        const int64_t g = s->n_rows;
        int shard;
        int64_t local;
        locate(s, g, &shard, &local);
        const int64_t take = std::min<int64_t>(s->B - g % s->B, n - done);
        int rc;
        if (record_mode) {
            rc = vg_corpus_append_records(s->sh[(size_t)shard], p + done * stride, take);
        } else {
            const int64_t *ids = rowids ? rowids + done : nullptr;
            if (!ids && s->S > 1) {                    // implicit rowids follow the GLOBAL position, not the shard's
                gen.resize((size_t)take);
                for (int64_t i = 0; i < take; ++i) gen[(size_t)i] = s->rowid_base + g + i;
                ids = gen.data();
            }
            rc = vg_corpus_append(s->sh[(size_t)shard], p + done * stride, take, stride, ids);
        }
        if (rc != VG_OK) return rc;
        s->n_rows += take;
        done += take;
    }
    return VG_OK;
}

extern "C" int vg_shards_append(vg_shards *s, const void *host_rows, int64_t n_rows, int64_t row_stride_bytes, const int64_t *rowids) {
    return append_common(s, host_rows, n_rows, row_stride_bytes, rowids, false);
}

extern "C" int vg_shards_append_records(vg_shards *s, const void *host_records, int64_t n_records) {
    if (!s) return fail(VG_ERR_INVALID, "shards handle is NULL");
    return append_common(s, host_records, n_records, 8 + (int64_t)s->dim, nullptr, true);
}

extern "C" int64_t vg_shards_rowid_at(const vg_shards *s, int64_t position) {
    if (!s || position < 0 || position >= s->n_rows) return 0;
    int shard;
    int64_t local;
    locate(s, position, &shard, &local);
    return vg_corpus_rowid_at(s->sh[(size_t)shard], local);
}

extern "C" int vg_shards_rowids(const vg_shards *s, int64_t pos0, int64_t n, int64_t *out) {
    if (!s || !out || pos0 < 0 || n < 0 || pos0 + n > s->n_rows) return fail(VG_ERR_INVALID, "vg_shards_rowids: bad range");
    int64_t g = pos0;
    while (g < pos0 + n) {                                   // block by block: one shard, consecutive local positions
        int shard;
        int64_t local;
        locate(s, g, &shard, &local);
        const int64_t take = std::min<int64_t>(s->B - g % s->B, pos0 + n - g);
        const vg_corpus *c = s->sh[(size_t)shard];
        for (int64_t i = 0; i < take; ++i) out[g - pos0 + i] = vg_corpus_rowid_at(c, local + i);
        g += take;
    }
    return VG_OK;
}

// Row maintenance (vg_corpus_patch_rows / _delete_rows / _find_rowid).  A deletion shifts every later row by one position, i.e.
// across the block-cyclic deal of several shards: only single-shard handles are served, the caller re-stages otherwise.
extern "C" int64_t vg_shards_find_rowid(const vg_shards *s, int64_t rowid) {
    if (!s) return -1;
    if (s->S != 1) return -2;
    return vg_corpus_find_rowid(s->sh[0], rowid);
}
extern "C" int vg_shards_patch_rows(vg_shards *s, const int64_t *positions, int64_t n, const void *host_rows, int64_t row_stride_bytes) {
    if (!s) return fail(VG_ERR_INVALID, "shards handle is NULL");
    if (s->S != 1) return fail(VG_ERR_UNSUPPORTED, "row maintenance needs a single-shard corpus");
    return vg_corpus_patch_rows(s->sh[0], positions, n, host_rows, row_stride_bytes);
}
extern "C" int vg_shards_delete_rows(vg_shards *s, const int64_t *positions, int64_t n) {
    if (!s) return fail(VG_ERR_INVALID, "shards handle is NULL");
    if (s->S != 1) return fail(VG_ERR_UNSUPPORTED, "row maintenance needs a single-shard corpus");
    int rc = vg_corpus_delete_rows(s->sh[0], positions, n);
    if (rc == VG_OK) s->n_rows = vg_corpus_rows(s->sh[0]);
    return rc;
}

extern "C" int vg_shards_set_scan_filter(vg_shards *s, int mode) {
    if (!s) return fail(VG_ERR_INVALID, "shards handle is NULL");
    for (auto *p : s->sh) {
        int rc = vg_corpus_set_scan_filter(p, mode);
        if (rc != VG_OK) return rc;
    }
    return VG_OK;
}

struct Cand { uint32_t img; int64_t gpos; int shard; uint32_t local; };

static inline bool cand_less(const Cand &a, const Cand &b) { return a.img != b.img ? a.img < b.img : a.gpos < b.gpos; }

// merge per-shard ascending key lists (list i = shard i at keys + i * pitch, counts[i * cpitch] keys valid) into the global top-k.
// ref_k >= 0: the lists were taken with one more slot than asked for (tie_order = reference, see vg_scan_topk_reference): when the
// best ref_k + 1 distances are pairwise distinct the reference's own result IS the first ref_k in ascending order and that is what
// comes back; when they hold a tie nothing is written and -1 comes back (the caller replays the reference's slots).
// out_gkeys (optional): the winners as keys over GLOBAL positions (distance image << 32 | global position; the paged scans' _keys forms).
static int merge_lists(const vg_shards *s, const uint64_t *keys, size_t pitch, const int *counts, int cpitch, int k, int64_t *out_rowids,
                       double *out_dist, int ref_k = -1, uint64_t *out_gkeys = nullptr) {
    std::vector<Cand> all;
    for (int i = 0; i < s->S; ++i)
        for (int j = 0; j < counts[(size_t)i * cpitch]; ++j) {
            const uint64_t key = keys[(size_t)i * pitch + j];
            if (key == VG_KEY_EMPTY) break;
            const uint32_t local = vg_key_position(key);
            all.push_back(Cand{(uint32_t)(key >> 32), global_of(s, i, (int64_t)local), i, local});
        }
    size_t take = std::min<size_t>((size_t)k, all.size());
    std::partial_sort(all.begin(), all.begin() + (long)take, all.end(), cand_less);
    if (ref_k >= 0) {
        for (size_t i = 1; i < take; ++i) if (all[i].img == all[i - 1].img) return -1;
        take = std::min<size_t>(take, (size_t)ref_k);
    }
    for (size_t i = 0; i < take; ++i) {
        out_dist[i] = (double)vg_key_distance((uint64_t)all[i].img << 32);
        out_rowids[i] = vg_corpus_rowid_at(s->sh[(size_t)all[i].shard], (int64_t)all[i].local);
        if (out_gkeys) out_gkeys[i] = ((uint64_t)all[i].img << 32) | (uint64_t)all[i].gpos;
    }
    return (int)take;
}
// the same for query q of a batch: keys [S][nq][kk], counts [S][nq]
static int merge_query_lists(const vg_shards *s, const uint64_t *keys, const int *counts, int nq, int q, int kk, int k, int64_t *out_rowids,
                             double *out_dist, int ref_k = -1, uint64_t *out_gkeys = nullptr) {
    return merge_lists(s, keys + (size_t)q * kk, (size_t)nq * kk, counts + q, nq, k, out_rowids, out_dist, ref_k, out_gkeys);
}

// ---- tie_order = reference over several shards: the same replay (vg_refslots.h), its stream assembled in GLOBAL scan
// order from the shards' resident distances
extern "C" int vg_shards_set_tie_order(vg_shards *s, int mode) {
    if (!s) return fail(VG_ERR_INVALID, "shards handle is NULL");
    for (auto *p : s->sh) {
        int rc = vg_corpus_set_tie_order(p, mode);
        if (rc != VG_OK) return rc;
    }
    s->tie_order = mode;
    return VG_OK;
}

// local rows of shard i in front of GLOBAL scan position g0: its whole blocks below block g0 / B, + g0 % B when that block is its own
static inline int64_t local_rows_before(const vg_shards *s, int i, int64_t g0) {
    const int64_t pb = g0 / s->B, rem = g0 % s->B;
    const int64_t full = (pb + s->S - 1 - i) / s->S;
    return full * s->B + ((int)(pb % s->S) == i ? rem : 0);
}

namespace {
struct ShardsSrc {
    vg_shards *s;
    std::vector<uint64_t> pairs;
    static const int64_t kCap = 1 << 17;
    int fetch(int64_t g0, int64_t cnt, float *out) {
        int64_t g = g0;
        while (g < g0 + cnt) {
            int shard;
            int64_t local;
            locate(s, g, &shard, &local);
            const int64_t take = std::min<int64_t>(s->B - g % s->B, g0 + cnt - g);
            int rc = vg_resident_distances_fetch(s->sh[(size_t)shard], local, take, out + (g - g0));
            if (rc != VG_OK) return rc;
            g += take;
        }
        return VG_OK;
    }
    int below(int64_t g0, float bound, std::vector<VgRefCand> &out, bool *overflow) {
        pairs.resize((size_t)kCap);
        for (int i = 0; i < s->S; ++i) {
            const int64_t local_from = local_rows_before(s, i, g0);
            int64_t count = 0;
            int rc = vg_resident_distances_below(s->sh[(size_t)i], local_from, bound, pairs.data(), kCap, &count);
            if (rc != VG_OK) return rc;
            if (count > kCap) { *overflow = true; return VG_OK; }
            for (int64_t j = 0; j < count; ++j)
                out.push_back(VgRefCand{global_of(s, i, vg_pair_position(pairs[(size_t)j])), vg_pair_distance(pairs[(size_t)j])});
        }
        return VG_OK;
    }
};
}

// the store-mode replay: every shard scans again leaving all its distances resident, the host replays a prefix and asks the shards
// for the later rows below the bound (vg_reforder.hip).  What is left for k > 64, rows too long for an emitting kernel and candidate
// streams that overflow.
static int shards_scan_topk_reference(vg_shards *s, int metric, const void *query, int k, int64_t *out_rowids, double *out_dist,
                                      int *out_count) {
    int rc = VG_OK;
    for (int i = 0; i < s->S && rc == VG_OK; ++i) rc = vg_scan_distances_resident(s->sh[(size_t)i], metric, query);   // all shards in flight
    if (rc != VG_OK) return rc;
    ShardsSrc src{s, {}};
    VgRefSlots slots;
    if ((rc = vg_ref_replay(src, s->n_rows, k, slots)) != VG_OK) return rc;
    const int cnt = slots.finish();
    for (int i = 0; i < cnt; ++i) {
        out_dist[i] = slots.dist[(size_t)i];
        out_rowids[i] = vg_shards_rowid_at(s, slots.pos[(size_t)i]);
    }
    *out_count = cnt;
    ++s->ref_stats[3];
    return VG_OK;
}

// The reference's slots replayed over what the shards' emitting launches left behind (vg_scan_topk_reference does the same for one
// corpus).  Every shard ran its own prefix pass over ITS first P_i rows and emitted, behind them, every row that beats the k-th best
// of the shard's EARLIER rows: local order is monotone in global order, so those rows precede the row globally too and the union of
// the shards' streams is a superset of the rows that can enter the slots.  Offering a row that cannot enter is a no-op, so replaying
// the union in GLOBAL scan order ends in exactly the reference's slots - no second scan, whatever the number of shards.
// *overflow: a shard's stream did not fit its buffer / a shard could not emit (the caller takes the store-mode replay).
static int shards_replay_emitted(vg_shards *s, int k, VgRefSlots &slots, bool *overflow) {
    struct Part { const float *prefix = nullptr; int64_t P = 0; unsigned long long *pairs = nullptr; unsigned long long count = 0; };
    std::vector<Part> parts((size_t)s->S);
    *overflow = false;
    for (int i = 0; i < s->S; ++i) {
        vg_corpus *c = s->sh[(size_t)i];
        if (c->n_rows == 0) continue;
        if (c->ref_prefix_rows <= 0) { *overflow = true; return VG_OK; }
        int rc = vg_ref_emitted_enqueue(c);                    // every shard's copies in flight before the first wait
        if (rc != VG_OK) return rc;
    }
    struct GCand { int64_t gpos; float d; };
    std::vector<GCand> cand;
    int64_t max_p = 0;
    for (int i = 0; i < s->S; ++i) {
        vg_corpus *c = s->sh[(size_t)i];
        if (c->n_rows == 0) continue;
        Part &pt = parts[(size_t)i];
        bool ovf = false;
        int rc = vg_ref_emitted_wait(c, &pt.prefix, &pt.P, &pt.pairs, &pt.count, &ovf);
        if (rc != VG_OK) return rc;
        if (ovf) *overflow = true;                             // (keep draining the other shards' streams: their copies are in flight)
        max_p = std::max(max_p, pt.P);
    }
    if (*overflow) return VG_OK;
    for (int i = 0; i < s->S; ++i) {
        const Part &pt = parts[(size_t)i];
        for (unsigned long long j = 0; j < pt.count; ++j) {
            const int64_t local = vg_pair_position(pt.pairs[j]);
            if (local >= pt.P) cand.push_back(GCand{global_of(s, i, local), vg_pair_distance(pt.pairs[j])});   // (the main pass covers the prefix rows again)
        }
    }
    std::sort(cand.begin(), cand.end(), [](const GCand &x, const GCand &y) { return x.gpos < y.gpos; });
    slots.init(k);
    // the prefixes, block by block in global order (local block lb of shard i is global block lb * S + i), the candidates in between
    size_t ci = 0;
    for (int64_t lb = 0; lb * s->B < max_p; ++lb)
        for (int i = 0; i < s->S; ++i) {
            const Part &pt = parts[(size_t)i];
            const int64_t l0 = lb * s->B;
            if (l0 >= pt.P) continue;
            const int64_t len = std::min<int64_t>(s->B, pt.P - l0);
            const int64_t g0 = global_of(s, i, l0);
            for (; ci < cand.size() && cand[ci].gpos < g0; ++ci) slots.offer(cand[ci].d, cand[ci].gpos);
            vg_ref_offer_run(slots, pt.prefix + l0, len, g0);
        }
    for (; ci < cand.size(); ++ci) slots.offer(cand[ci].d, cand[ci].gpos);
    return VG_OK;
}

// Every shard's fused top-k scan (kk <= 64 list slots) and its 64 candidate keys on the host, S x 64.  The RCCL gather where the handle
// asks for it and it serves (not an emitting scan: that leaves more than 64 keys behind) - a failure there leaves the host gather to
// this query and the ones after it; host gather: every shard in flight before the first wait, or each on its own pool thread.
static int scan_shards_topk(vg_shards *s, int metric, const void *query, int kk, bool emit, uint64_t *keys) {
    if (!emit && s->gather_mode == 1 && rccl_ready(s)) {
        if (rccl_scan_and_gather(s, metric, query, kk, keys) == VG_OK) return VG_OK;
        s->rccl_failed = true;
    }
    int rc = VG_OK;
    if (s->threaded) {
        rc = pool_run(s, [&](int i) {
            const int r = vg_scan_topk_enqueue_plan(s->sh[(size_t)i], metric, query, kk, emit);
            return r != VG_OK ? r : vg_scan_topk_collect(s->sh[(size_t)i], &keys[(size_t)i * VG_WAVE_KEYS]);
        });
    } else {
        for (int i = 0; i < s->S && rc == VG_OK; ++i) rc = vg_scan_topk_enqueue_plan(s->sh[(size_t)i], metric, query, kk, emit);
        for (int i = 0; i < s->S; ++i) {
            int rc2 = vg_scan_topk_collect(s->sh[(size_t)i], &keys[(size_t)i * VG_WAVE_KEYS]);
            if (rc == VG_OK) rc = rc2;
        }
    }
    if (rc == VG_OK) ++s->gather_calls[0];
    return rc;
}

// tie_order = reference for k <= 64 over several shards, the fused form: every shard's ordinary top-k scan with one more list slot;
// a tie among the merged k + 1 best -> the replay above.  The policy is one corpus' (vg_scan_topk_reference): scans through a filter
// kernel always emit, plain-kernel scans only while ties are around (a first tie costs one more scan of every shard, emitting);
// k = 64 has no 65th slot: it runs emitting with k slots and always replays.
static int shards_scan_topk_fused(vg_shards *s, int metric, const void *query, int k, bool force_emit, int64_t *out_rowids,
                                  double *out_dist, int *out_count) {
    ++s->ref_stats[0];
    const bool always = (k == VG_WAVE_KEYS);
    const int kk = always ? k : k + 1;
    vg_corpus *probe = nullptr;
    for (auto *c : s->sh) if (c->n_rows > 0) { probe = c; break; }
    bool emit = force_emit || always || s->ref_hot > 0 || (probe && vg_scan_filter_would_serve(probe, metric, kk));
    std::vector<uint64_t> keys((size_t)s->S * VG_WAVE_KEYS);
    std::vector<int> counts((size_t)s->S, VG_WAVE_KEYS);
    for (int attempt = 0; attempt < 2; ++attempt) {
        int rc = scan_shards_topk(s, metric, query, kk, emit, keys.data());
        if (rc != VG_OK) return rc;
        if (!always) {
            const int got = merge_lists(s, keys.data(), VG_WAVE_KEYS, counts.data(), 1, kk, out_rowids, out_dist, k);
            if (got >= 0) {
                *out_count = got;
                if (s->ref_hot > 0) --s->ref_hot;
                return VG_OK;
            }
            s->ref_hot = 16;
        }
        if (attempt == 0) ++s->ref_stats[1];
        if (emit) {
            VgRefSlots slots;
            bool overflow = false;
            rc = shards_replay_emitted(s, k, slots, &overflow);
            if (rc != VG_OK) return rc;
            if (overflow) break;
            const int n = slots.finish();
            for (int i = 0; i < n; ++i) {
                out_dist[i] = slots.dist[(size_t)i];
                out_rowids[i] = vg_shards_rowid_at(s, slots.pos[(size_t)i]);
            }
            *out_count = n;
            ++s->ref_stats[2];
            return VG_OK;
        }
        emit = true;                                               // a tie and nothing emitted: scan again, emitting
    }
    return shards_scan_topk_reference(s, metric, query, k, out_rowids, out_dist, out_count);
}

extern "C" int vg_corpus_device_bytes(const vg_corpus *c, long long *out3);
extern "C" int vg_shards_device_bytes(const vg_shards *s, long long *out3) {
    if (!s || !out3) return fail(VG_ERR_INVALID, "vg_shards_device_bytes: NULL argument");
    out3[0] = out3[1] = out3[2] = 0;
    for (int i = 0; i < s->S; ++i) {
        long long one[3] = {0, 0, 0};
        const int rc = vg_corpus_device_bytes(s->sh[(size_t)i], one);
        if (rc != VG_OK) return rc;
        for (int j = 0; j < 3; ++j) out3[j] += one[j];
    }
    return VG_OK;
}

extern "C" int vg_shards_threaded(const vg_shards *s) { return s ? s->threaded : 0; }

extern "C" int vg_shards_tie_stats(const vg_shards *s, unsigned long long *out4) {
    if (!s || !out4) return fail(VG_ERR_INVALID, "vg_shards_tie_stats: NULL argument");
    if (s->S == 1) return vg_corpus_tie_stats(s->sh[0], out4);
    for (int i = 0; i < 4; ++i) out4[i] = s->ref_stats[i];
    return VG_OK;
}

extern "C" int vg_shards_scan_topk(vg_shards *s, int metric, const void *query, int k, int64_t *out_rowids, double *out_dist,
                                   int *out_count) {
    if (!s || !query || !out_count) return fail(VG_ERR_INVALID, "vg_shards_scan_topk: NULL argument");
    *out_count = 0;
    if (s->S == 1 && s->gather_mode == 0) return vg_scan_topk(s->sh[0], metric, query, k, out_rowids, out_dist, out_count);
    if (k <= 0 || s->n_rows == 0) return VG_OK;
    if (!out_rowids || !out_dist) return fail(VG_ERR_INVALID, "vg_shards_scan_topk: NULL output");
    if (int rcm = vg_metric_check_tie(s->vtype, metric, s->tie_order, "vg_shards_scan_topk")) return rcm;
    const bool ref = s->tie_order == VG_TIE_REFERENCE;
    if (ref && k > VG_WAVE_KEYS) { ++s->ref_stats[0]; return shards_scan_topk_reference(s, metric, query, k, out_rowids, out_dist, out_count); }
    if (ref) return shards_scan_topk_fused(s, metric, query, k, false, out_rowids, out_dist, out_count);
    if (k <= VG_WAVE_KEYS) {
        std::vector<uint64_t> keys((size_t)s->S * VG_WAVE_KEYS);
        std::vector<int> counts((size_t)s->S, VG_WAVE_KEYS);
        int rc = scan_shards_topk(s, metric, query, k, false, keys.data());
        if (rc != VG_OK) return rc;
        *out_count = merge_lists(s, keys.data(), VG_WAVE_KEYS, counts.data(), 1, k, out_rowids, out_dist);
        return VG_OK;
    }
    const int kk = (int)std::min<int64_t>((int64_t)k, s->n_rows);
    std::vector<uint64_t> keys((size_t)s->S * kk);
    std::vector<int> counts((size_t)s->S, 0);
    int rc = for_each_shard(s, [&](int i) {
        return vg_scan_topk_keys(s->sh[(size_t)i], metric, query, kk, &keys[(size_t)i * kk], &counts[(size_t)i]);
    });
    if (rc != VG_OK) return rc;
    *out_count = merge_lists(s, keys.data(), kk, counts.data(), 1, kk, out_rowids, out_dist);
    return VG_OK;
}

extern "C" int vg_shards_scan_topk_batch(vg_shards *s, int metric, const void *queries, int nq, int k, int64_t *out_rowids,
                                         double *out_dist, int *out_counts) {
    if (!s || !queries || !out_counts) return fail(VG_ERR_INVALID, "vg_shards_scan_topk_batch: NULL argument");
    if (s->S == 1) return vg_scan_topk_batch(s->sh[0], metric, queries, nq, k, out_rowids, out_dist, out_counts);
    if (nq <= 0) return VG_OK;
    for (int i = 0; i < nq; ++i) out_counts[i] = 0;
    if (k <= 0 || s->n_rows == 0) return VG_OK;
    if (!out_rowids || !out_dist) return fail(VG_ERR_INVALID, "vg_shards_scan_topk_batch: NULL output");
    if (int rcm = vg_metric_check_tie(s->vtype, metric, s->tie_order, "vg_shards_scan_topk_batch")) return rcm;
    const bool ref = s->tie_order == VG_TIE_REFERENCE;      // (one more list slot; only the queries with a tie are answered again, one by one)
    const size_t qbytes = (size_t)s->dim * s->es;
    if (ref && k >= VG_WAVE_KEYS) {                          // no slot to look for a tie with: every query through the single-query form
        for (int q = 0; q < nq; ++q) {
            int rc1 = vg_shards_scan_topk(s, metric, (const uint8_t *)queries + (size_t)q * qbytes, k, out_rowids + (size_t)q * k,
                                          out_dist + (size_t)q * k, &out_counts[q]);
            if (rc1 != VG_OK) return rc1;
        }
        return VG_OK;
    }
    // f32 rows on the f32 matrix cores sum in another order than the single scans the reference order is defined on: a tie under the
    // single scan's arithmetic could go unnoticed in the batch's keys - such batches are answered query by query
    if (ref && s->vtype == VG_TYPE_F32 && !vg_batch_keys_are_scan_exact(s->sh[0], metric, k + 1)) {
        for (int q = 0; q < nq; ++q) {
            int rc1 = shards_scan_topk_fused(s, metric, (const uint8_t *)queries + (size_t)q * qbytes, k, false, out_rowids + (size_t)q * k,
                                             out_dist + (size_t)q * k, &out_counts[q]);
            if (rc1 != VG_OK) return rc1;
        }
        return VG_OK;
    }
    const int kk = (int)std::min<int64_t>((int64_t)k + (ref ? 1 : 0), s->n_rows);
    std::vector<uint64_t> keys((size_t)s->S * nq * kk);
    std::vector<int> counts((size_t)s->S * nq, 0);
    int rc = for_each_shard(s, [&](int i) {
        return vg_scan_topk_batch_keys(s->sh[(size_t)i], metric, queries, nq, kk, &keys[(size_t)i * nq * kk], &counts[(size_t)i * nq]);
    });
    if (rc != VG_OK) return rc;
    for (int q = 0; q < nq; ++q) {
        int got = merge_query_lists(s, keys.data(), counts.data(), nq, q, kk, kk, out_rowids + (size_t)q * k, out_dist + (size_t)q * k, ref ? k : -1);
        if (got < 0) {                                       // a tie: this query again through the emitting scans + the replay
            int rc1 = shards_scan_topk_fused(s, metric, (const uint8_t *)queries + (size_t)q * qbytes, k, true, out_rowids + (size_t)q * k,
                                             out_dist + (size_t)q * k, &got);
            if (rc1 != VG_OK) return rc1;
        }
        out_counts[q] = got;
    }
    return VG_OK;
}

extern "C" int vg_shards_scan_distances(vg_shards *s, int metric, const void *query, float *out_dist_host) {
    if (!s || !query || !out_dist_host) return fail(VG_ERR_INVALID, "vg_shards_scan_distances: NULL argument");
    if (s->S == 1) return vg_scan_distances(s->sh[0], metric, query, out_dist_host);
    if (s->n_rows == 0) return VG_OK;
    return for_each_shard(s, [&](int i) {
        vg_corpus *c = s->sh[(size_t)i];
        const int64_t n = vg_corpus_rows(c);
        if (n == 0) return (int)VG_OK;
        std::vector<float> tmp((size_t)n);
        int rc = vg_scan_distances(c, metric, query, tmp.data());
        if (rc != VG_OK) return rc;
        for (int64_t l0 = 0; l0 < n; l0 += s->B) {                                   // local block -> its global place
            const int64_t len = std::min<int64_t>(s->B, n - l0);
            memcpy(out_dist_host + global_of(s, i, l0), &tmp[(size_t)l0], (size_t)len * sizeof(float));
        }
        return (int)VG_OK;
    });
}

// ---- range scans: every shard runs vg_scan_within (same radius, same limit - the first `limit` of the whole are among the first `limit`
// of every shard); local order is monotone in global order, so sorting the held keys by (distance image, global position) is the order
// of one corpus holding all rows.  The single and the batch form share the merge and the fetch.

// the shards' held keys of one query (read_keys(shard, n, out) brings shard's n) -> hits: merged, cut to `limit`.  matches / held: one
// count per shard, `pitch` apart.  Returns VG_OK with *out_total = the matches of all shards.
template <typename ReadKeys>
static int merge_within(const vg_shards *s, const int64_t *matches, const int64_t *held, size_t pitch, int64_t limit, ReadKeys read_keys,
                        std::vector<vg_shards::WithinHit> *hits, int64_t *out_total) {
    int64_t total = 0;
    std::vector<uint64_t> keys;
    hits->clear();
    for (int i = 0; i < s->S; ++i) {
        total += matches[(size_t)i * pitch];
        keys.resize((size_t)held[(size_t)i * pitch]);
        int rc = read_keys(i, (int64_t)keys.size(), keys.data());
        if (rc != VG_OK) return rc;
        for (uint64_t key : keys) hits->push_back(vg_shards::WithinHit{key, global_of(s, i, (int64_t)vg_key_position(key)), i});
    }
    std::sort(hits->begin(), hits->end(), [](const vg_shards::WithinHit &a, const vg_shards::WithinHit &b) {
        const uint32_t ia = (uint32_t)(a.key >> 32), ib = (uint32_t)(b.key >> 32);
        return ia != ib ? ia < ib : a.gpos < b.gpos;
    });
    const int64_t keep = (limit > 0) ? std::min<int64_t>(limit, total) : total;
    if ((int64_t)hits->size() > keep) hits->resize((size_t)keep);
    *out_total = total;
    return VG_OK;
}

// rows [first, first + n) of a merged result
static int fetch_within(const vg_shards *s, const char *who, const std::vector<vg_shards::WithinHit> &hits, int64_t first, int64_t n,
                        int64_t *out_rowids, double *out_dist) {
    if (n < 0) n = 0;
    if (first < 0 || first + n > (int64_t)hits.size()) return fail(VG_ERR_INVALID, (std::string(who) + ": rows outside the held result").c_str());
    for (int64_t i = 0; i < n; ++i) {
        const vg_shards::WithinHit &h = hits[(size_t)(first + i)];
        if (out_rowids) out_rowids[i] = vg_corpus_rowid_at(s->sh[(size_t)h.shard], (int64_t)vg_key_position(h.key));
        if (out_dist) out_dist[i] = (double)vg_key_distance(h.key);
    }
    return VG_OK;
}

// which range form a call over shards stands for: whose names errors carry (the shards' entry point, the per-corpus one), and what
// every shard must hold - a mask (masked forms: every shard over its own bits; a shard whose share of the mask is empty launches
// nothing), labels (labeled forms: labels mean the same on every shard) or values (the valued form: so does an interval)
struct WithinShardForm { const char *who; const char *inner; bool masked; bool labeled; bool valued; };

static int within_shard_refusal(const vg_shards *s, const WithinShardForm &f) {
    if (f.masked && vg_shards_mask_count(s) < 0) return fail(VG_ERR_INVALID, (std::string(f.inner) + ": no row mask set").c_str());
    if (f.labeled && !vg_shards_has_labels(s)) return fail(VG_ERR_INVALID, (std::string(f.inner) + ": no labels set").c_str());
    if (f.valued && !vg_shards_has_values(s)) return fail(VG_ERR_INVALID, (std::string(f.inner) + ": no values set").c_str());
    return VG_OK;
}

// the single forms; scan(corpus, out_matches, out_held): the form's range scan over one shard
template <typename Scan>
static int shards_within(vg_shards *s, const WithinShardForm &f, const void *query, int64_t limit, int64_t *out_matches, int64_t *out_held, Scan scan) {
    if (out_matches) *out_matches = 0;
    if (out_held) *out_held = 0;
    if (!s || !query) return fail(VG_ERR_INVALID, (std::string(f.who) + ": NULL argument").c_str());
    if (s->S == 1) return scan(s->sh[0], out_matches, out_held);
    s->within_hits.clear();
    int rc = within_shard_refusal(s, f);
    if (rc != VG_OK) return rc;
    std::vector<int64_t> matches((size_t)s->S, 0), held((size_t)s->S, 0);
    rc = for_each_shard(s, [&](int i) { return scan(s->sh[(size_t)i], &matches[(size_t)i], &held[(size_t)i]); });
    if (rc != VG_OK) return rc;
    int64_t total = 0;
    rc = merge_within(s, matches.data(), held.data(), 1, limit,
                      [&](int i, int64_t n, uint64_t *out) { return vg_scan_within_keys(s->sh[(size_t)i], 0, n, out); }, &s->within_hits, &total);
    if (rc != VG_OK) return rc;
    if (out_matches) *out_matches = total;
    if (out_held) *out_held = (int64_t)s->within_hits.size();
    return VG_OK;
}

extern "C" int vg_shards_scan_within(vg_shards *s, int metric, const void *query, double radius, int64_t limit, int64_t *out_matches,
                                     int64_t *out_held) {
    const WithinShardForm f = {"vg_shards_scan_within", "vg_scan_within", false, false};
    return shards_within(s, f, query, limit, out_matches, out_held,
                         [&](vg_corpus *c, int64_t *m, int64_t *h) { return vg_scan_within(c, metric, query, radius, limit, m, h); });
}

extern "C" int vg_shards_scan_within_masked(vg_shards *s, int metric, const void *query, double radius, int64_t limit, int64_t *out_matches,
                                            int64_t *out_held) {
    const WithinShardForm f = {"vg_shards_scan_within_masked", "vg_scan_within_masked", true, false};
    return shards_within(s, f, query, limit, out_matches, out_held,
                         [&](vg_corpus *c, int64_t *m, int64_t *h) { return vg_scan_within_masked(c, metric, query, radius, limit, m, h); });
}

extern "C" int vg_shards_scan_within_labeled(vg_shards *s, int metric, const void *query, double radius, int64_t limit, uint32_t label,
                                             int64_t *out_matches, int64_t *out_held) {
    const WithinShardForm f = {"vg_shards_scan_within_labeled", "vg_scan_within_labeled", false, true};
    return shards_within(s, f, query, limit, out_matches, out_held,
                         [&](vg_corpus *c, int64_t *m, int64_t *h) { return vg_scan_within_labeled(c, metric, query, radius, limit, label, m, h); });
}

extern "C" int vg_shards_scan_within_labelset(vg_shards *s, int metric, const void *query, double radius, int64_t limit, const uint32_t *labels,
                                              int64_t n_labels, int exclude, int64_t *out_matches, int64_t *out_held) {
    const WithinShardForm f = {"vg_shards_scan_within_labelset", "vg_scan_within_labelset", false, true};
    return shards_within(s, f, query, limit, out_matches, out_held, [&](vg_corpus *c, int64_t *m, int64_t *h) {
        return vg_scan_within_labelset(c, metric, query, radius, limit, labels, n_labels, exclude, m, h);
    });
}

extern "C" int vg_shards_scan_within_valued(vg_shards *s, int metric, const void *query, double radius, int64_t limit, int64_t lo, int64_t hi,
                                            int64_t *out_matches, int64_t *out_held) {
    const WithinShardForm f = {"vg_shards_scan_within_valued", "vg_scan_within_valued", false, false, true};
    return shards_within(s, f, query, limit, out_matches, out_held,
                         [&](vg_corpus *c, int64_t *m, int64_t *h) { return vg_scan_within_valued(c, metric, query, radius, limit, lo, hi, m, h); });
}

extern "C" int vg_shards_scan_within_fetch(const vg_shards *s, int64_t first, int64_t n, int64_t *out_rowids, double *out_dist) {
    if (!s) return fail(VG_ERR_INVALID, "vg_shards_scan_within_fetch: NULL argument");
    if (s->S == 1) return vg_scan_within_fetch(s->sh[0], first, n, out_rowids, out_dist);
    if (n <= 0) return VG_OK;
    return fetch_within(s, "vg_shards_scan_within_fetch", s->within_hits, first, n, out_rowids, out_dist);
}

extern "C" int vg_shards_within_set_initial_capacity(vg_shards *s, int64_t keys) {
    if (!s) return fail(VG_ERR_INVALID, "vg_shards_within_set_initial_capacity: NULL argument");
    for (auto *c : s->sh) { int rc = vg_within_set_initial_capacity(c, keys); if (rc != VG_OK) return rc; }
    return VG_OK;
}

extern "C" int vg_shards_within_last_launches(const vg_shards *s) {
    int most = 0;
    if (s) for (auto *c : s->sh) most = std::max(most, vg_within_last_launches(c));
    return most;
}

// ---- batch range scans: every shard answers all nq queries (the form's batch range scan: same radii, same limit, same labels), then
// merge_within per query.  scan(corpus, out_matches, out_held): that scan over one shard
template <typename Scan>
static int shards_within_batch(vg_shards *s, const WithinShardForm &f, const void *queries, int nq, const double *radii, const void *extra,
                               int64_t limit, int64_t *out_matches, int64_t *out_held, Scan scan) {
    for (int q = 0; q < nq; ++q) { if (out_matches) out_matches[q] = 0; if (out_held) out_held[q] = 0; }
    if (!s || !queries || !radii || !extra) return fail(VG_ERR_INVALID, (std::string(f.who) + ": NULL argument").c_str());
    if (s->S == 1) return scan(s->sh[0], out_matches, out_held);
    s->within_batch_hits.clear();
    if (nq < 1) return fail(VG_ERR_INVALID, (std::string(f.inner) + ": nq must be at least 1").c_str());
    int rc = within_shard_refusal(s, f);
    if (rc != VG_OK) return rc;
    std::vector<int64_t> matches((size_t)s->S * nq, 0), held((size_t)s->S * nq, 0);
    rc = for_each_shard(s, [&](int i) { return scan(s->sh[(size_t)i], &matches[(size_t)i * nq], &held[(size_t)i * nq]); });
    if (rc != VG_OK) return rc;
    s->within_batch_hits.resize((size_t)nq);
    for (int q = 0; q < nq; ++q) {
        int64_t total = 0;
        rc = merge_within(s, &matches[(size_t)q], &held[(size_t)q], (size_t)nq, limit,
                          [&](int i, int64_t n, uint64_t *out) { return vg_scan_within_batch_keys(s->sh[(size_t)i], q, 0, n, out); },
                          &s->within_batch_hits[(size_t)q], &total);
        if (rc != VG_OK) { s->within_batch_hits.clear(); return rc; }
        if (out_matches) out_matches[q] = total;
        if (out_held) out_held[q] = (int64_t)s->within_batch_hits[(size_t)q].size();
    }
    return VG_OK;
}

extern "C" int vg_shards_scan_within_batch(vg_shards *s, int metric, const void *queries, int nq, const double *radii, int64_t limit,
                                           int64_t *out_matches, int64_t *out_held) {
    const WithinShardForm f = {"vg_shards_scan_within_batch", "vg_scan_within_batch", false, false};
    return shards_within_batch(s, f, queries, nq, radii, radii, limit, out_matches, out_held,
                               [&](vg_corpus *c, int64_t *m, int64_t *h) { return vg_scan_within_batch(c, metric, queries, nq, radii, limit, m, h); });
}

extern "C" int vg_shards_scan_within_batch_masked(vg_shards *s, int metric, const void *queries, int nq, const double *radii, int64_t limit,
                                                  int64_t *out_matches, int64_t *out_held) {
    const WithinShardForm f = {"vg_shards_scan_within_batch_masked", "vg_scan_within_batch_masked", true, false};
    return shards_within_batch(s, f, queries, nq, radii, radii, limit, out_matches, out_held,
                               [&](vg_corpus *c, int64_t *m, int64_t *h) { return vg_scan_within_batch_masked(c, metric, queries, nq, radii, limit, m, h); });
}

extern "C" int vg_shards_scan_within_batch_labeled(vg_shards *s, int metric, const void *queries, int nq, const uint32_t *query_labels,
                                                   const double *radii, int64_t limit, int64_t *out_matches, int64_t *out_held) {
    const WithinShardForm f = {"vg_shards_scan_within_batch_labeled", "vg_scan_within_batch_labeled", false, true};
    return shards_within_batch(s, f, queries, nq, radii, query_labels, limit, out_matches, out_held, [&](vg_corpus *c, int64_t *m, int64_t *h) {
        return vg_scan_within_batch_labeled(c, metric, queries, nq, query_labels, radii, limit, m, h);
    });
}

extern "C" int vg_shards_scan_within_batch_fetch(const vg_shards *s, int query, int64_t first, int64_t n, int64_t *out_rowids, double *out_dist) {
    if (!s) return fail(VG_ERR_INVALID, "vg_shards_scan_within_batch_fetch: NULL argument");
    if (s->S == 1) return vg_scan_within_batch_fetch(s->sh[0], query, first, n, out_rowids, out_dist);
    if (query < 0 || (size_t)query >= s->within_batch_hits.size()) return fail(VG_ERR_INVALID, "vg_shards_scan_within_batch_fetch: query outside the held result");
    return fetch_within(s, "vg_shards_scan_within_batch_fetch", s->within_batch_hits[(size_t)query], first, n, out_rowids, out_dist);
}

extern "C" int vg_shards_within_batch_plan(const vg_shards *s, int metric, int *out_queries_per_pass, int *out_lpr, int *out_u) {
    if (!s) return fail(VG_ERR_INVALID, "vg_shards_within_batch_plan: NULL argument");
    return vg_within_batch_plan(s->sh[0], metric, out_queries_per_pass, out_lpr, out_u);
}

extern "C" int vg_shards_within_batch_masked_plan(const vg_shards *s, int metric, int *out_queries_per_pass, int *out_lpr, int *out_u) {
    if (!s) return fail(VG_ERR_INVALID, "vg_shards_within_batch_masked_plan: NULL argument");
    return vg_within_batch_masked_plan(s->sh[0], metric, out_queries_per_pass, out_lpr, out_u);
}

extern "C" int vg_shards_within_batch_labeled_plan(const vg_shards *s, int metric, int *out_queries_per_pass, int *out_lpr, int *out_u) {
    if (!s) return fail(VG_ERR_INVALID, "vg_shards_within_batch_labeled_plan: NULL argument");
    return vg_within_batch_labeled_plan(s->sh[0], metric, out_queries_per_pass, out_lpr, out_u);
}

extern "C" int vg_shards_within_batch_set_initial_capacity(vg_shards *s, int64_t keys_per_query) {
    if (!s) return fail(VG_ERR_INVALID, "vg_shards_within_batch_set_initial_capacity: NULL argument");
    for (auto *c : s->sh) { int rc = vg_within_batch_set_initial_capacity(c, keys_per_query); if (rc != VG_OK) return rc; }
    return VG_OK;
}

extern "C" int vg_shards_within_batch_last_launches(const vg_shards *s) {
    int most = 0;
    if (s) for (auto *c : s->sh) most = std::max(most, vg_within_batch_last_launches(c));
    return most;
}

// ---- masked scans: the mask is given over GLOBAL scan positions and dealt out by the block-cyclic map of the rows (block b of B rows
// -> shard b % S, local rows (b / S) * B ...); every shard runs vg_scan_topk_masked over its own bits and the lists merge like the plain
// scan's, by (distance image, global position)
static inline uint64_t bits_at(const uint64_t *w, int64_t n_bits, int64_t pos, int n) {       // n <= 64 bits from `pos` on, 0 behind n_bits
    if (pos >= n_bits) return 0ull;
    const int64_t i = pos >> 6;
    const int sh = (int)(pos & 63);
    uint64_t v = w[i] >> sh;
    if (sh && ((i + 1) << 6) < n_bits) v |= w[i + 1] << (64 - sh);
    const int64_t have = std::min<int64_t>(n, n_bits - pos);
    return have >= 64 ? v : (v & ((1ull << have) - 1ull));
}
static inline void bits_put(uint64_t *w, int64_t pos, int n, uint64_t v) {                     // into zeroed words
    const int64_t i = pos >> 6;
    const int sh = (int)(pos & 63);
    w[i] |= v << sh;
    if (sh && sh + n > 64) w[i + 1] |= v >> (64 - sh);
}

// every shard's local words become its mask; a failure on the way leaves NO shard with a mask (never a mix of the new and the old one)
static int install_shard_masks(vg_shards *s, std::vector<std::vector<uint64_t>> &local, int64_t *out_set) {
    int64_t total = 0;
    for (int i = 0; i < s->S; ++i) {
        int rc = vg_corpus_set_mask_bits(s->sh[(size_t)i], local[(size_t)i].data(), vg_corpus_rows(s->sh[(size_t)i]));
        if (rc != VG_OK) {
            const std::string msg = vg_last_error();
            for (auto *c : s->sh) vg_corpus_clear_mask(c);
            return fail(rc, msg.c_str());
        }
        total += vg_corpus_mask_count(s->sh[(size_t)i]);
    }
    if (out_set) *out_set = total;
    return VG_OK;
}

extern "C" int vg_shards_set_mask_bits(vg_shards *s, const uint64_t *words, int64_t n_bits) {
    if (!s) return fail(VG_ERR_INVALID, "shards handle is NULL");
    if (s->S == 1) return vg_corpus_set_mask_bits(s->sh[0], words, n_bits);
    if (n_bits < 0 || (n_bits > 0 && !words) || n_bits > s->n_rows) return fail(VG_ERR_INVALID, "vg_shards_set_mask_bits: bad words pointer / bit count");
    std::vector<std::vector<uint64_t>> local((size_t)s->S);
    for (int i = 0; i < s->S; ++i) local[(size_t)i].assign((size_t)((vg_corpus_rows(s->sh[(size_t)i]) + 63) / 64) + 1, 0ull);
    for (int64_t g = 0; g < n_bits; g += s->B) {                               // block by block: one shard, consecutive local positions
        int shard;
        int64_t l0;
        locate(s, g, &shard, &l0);
        const int64_t len = std::min<int64_t>(s->B, n_bits - g);
        for (int64_t o = 0; o < len; o += 64) {
            const int n = (int)std::min<int64_t>(64, len - o);
            const uint64_t v = bits_at(words, n_bits, g + o, n);
            if (v) bits_put(local[(size_t)shard].data(), l0 + o, n, v);
        }
    }
    return install_shard_masks(s, local, nullptr);
}

extern "C" int vg_shards_set_mask_rowids(vg_shards *s, const int64_t *rowids, int64_t n, int64_t *out_set) {
    if (!s) return fail(VG_ERR_INVALID, "shards handle is NULL");
    if (s->S == 1) return vg_corpus_set_mask_rowids(s->sh[0], rowids, n, out_set);
    if (out_set) *out_set = 0;
    if (n < 0 || (n > 0 && !rowids)) return fail(VG_ERR_INVALID, "vg_shards_set_mask_rowids: bad rowids pointer / count");
    std::vector<std::vector<uint64_t>> local((size_t)s->S);
    for (int i = 0; i < s->S; ++i) local[(size_t)i].assign((size_t)((vg_corpus_rows(s->sh[(size_t)i]) + 63) / 64) + 1, 0ull);
    for (int i = 0; i < s->S; ++i)                                             // (decided before any rowid is looked at, like one corpus does)
        if (vg_corpus_find_rowid(s->sh[(size_t)i], 0) == -2)
            return fail(VG_ERR_UNSUPPORTED, "vg_shards_set_mask_rowids: the rowids are not ascending (no rowid lookup); set the mask by scan position");
    for (int64_t j = 0; j < n; ++j)
        for (int i = 0; i < s->S; ++i) {                                       // (every shard keeps its own rowid map: S bisections per rowid)
            const int64_t p = vg_corpus_find_rowid(s->sh[(size_t)i], rowids[j]);
            if (p >= 0) { local[(size_t)i][(size_t)(p >> 6)] |= 1ull << (p & 63); break; }
        }
    return install_shard_masks(s, local, out_set);
}

extern "C" int vg_shards_clear_mask(vg_shards *s) {
    if (!s) return fail(VG_ERR_INVALID, "shards handle is NULL");
    for (auto *c : s->sh) { int rc = vg_corpus_clear_mask(c); if (rc != VG_OK) return rc; }
    return VG_OK;
}

// rows allowed over all shards; -1 when a shard has no mask (an append drops the mask of the shards it reaches)
extern "C" int64_t vg_shards_mask_count(const vg_shards *s) {
    if (!s) return -1;
    int64_t total = 0;
    for (auto *c : s->sh) { const int64_t n = vg_corpus_mask_count(c); if (n < 0) return -1; total += n; }
    return total;
}

// ---- labels: given over GLOBAL scan positions and dealt out by the block-cyclic map of the rows, like the mask
extern "C" int vg_shards_set_labels(vg_shards *s, const uint32_t *labels, int64_t n) {
    if (!s) return fail(VG_ERR_INVALID, "shards handle is NULL");
    if (s->S == 1) return vg_corpus_set_labels(s->sh[0], labels, n);
    if (n != s->n_rows) return fail(VG_ERR_INVALID, "vg_shards_set_labels: the label count must equal the rows held");
    if (n > 0 && !labels) return fail(VG_ERR_INVALID, "vg_shards_set_labels: labels is NULL");
    std::vector<std::vector<uint32_t>> local((size_t)s->S);
    for (int i = 0; i < s->S; ++i) local[(size_t)i].assign((size_t)vg_corpus_rows(s->sh[(size_t)i]), VG_LABEL_NONE);
    for (int64_t g = 0; g < n; g += s->B) {                                    // block by block: one shard, consecutive local positions
        int shard;
        int64_t l0;
        locate(s, g, &shard, &l0);
        const int64_t len = std::min<int64_t>(s->B, n - g);
        if (l0 + len > (int64_t)local[(size_t)shard].size()) return fail(VG_ERR_INVALID, "vg_shards_set_labels: the shards do not hold the rows of the map");
        memcpy(local[(size_t)shard].data() + l0, labels + g, (size_t)len * sizeof(uint32_t));
    }
    for (int i = 0; i < s->S; ++i) {                   // a failure on the way leaves NO shard with labels
        int rc = vg_corpus_set_labels(s->sh[(size_t)i], local[(size_t)i].data(), (int64_t)local[(size_t)i].size());
        if (rc != VG_OK) {
            const std::string msg = vg_last_error();
            for (auto *c : s->sh) vg_corpus_clear_labels(c);
            return fail(rc, msg.c_str());
        }
    }
    return VG_OK;
}

extern "C" int vg_shards_clear_labels(vg_shards *s) {
    if (!s) return fail(VG_ERR_INVALID, "shards handle is NULL");
    for (auto *c : s->sh) { int rc = vg_corpus_clear_labels(c); if (rc != VG_OK) return rc; }
    return VG_OK;
}

// 1 while every shard holds labels (an append drops the labels of the shards it reaches)
extern "C" int vg_shards_has_labels(const vg_shards *s) {
    if (!s) return 0;
    for (auto *c : s->sh) if (!vg_corpus_has_labels(c)) return 0;
    return 1;
}

// ---- values: given over GLOBAL scan positions and dealt out like the labels
extern "C" int vg_shards_set_values(vg_shards *s, const int64_t *values, int64_t n) {
    if (!s) return fail(VG_ERR_INVALID, "shards handle is NULL");
    if (s->S == 1) return vg_corpus_set_values(s->sh[0], values, n);
    if (n != s->n_rows) return fail(VG_ERR_INVALID, "vg_shards_set_values: the value count must equal the rows held");
    if (n > 0 && !values) return fail(VG_ERR_INVALID, "vg_shards_set_values: values is NULL");
    std::vector<std::vector<int64_t>> local((size_t)s->S);
    for (int i = 0; i < s->S; ++i) local[(size_t)i].assign((size_t)vg_corpus_rows(s->sh[(size_t)i]), 0);
    for (int64_t g = 0; g < n; g += s->B) {                                    // block by block: one shard, consecutive local positions
        int shard;
        int64_t l0;
        locate(s, g, &shard, &l0);
        const int64_t len = std::min<int64_t>(s->B, n - g);
        if (l0 + len > (int64_t)local[(size_t)shard].size()) return fail(VG_ERR_INVALID, "vg_shards_set_values: the shards do not hold the rows of the map");
        memcpy(local[(size_t)shard].data() + l0, values + g, (size_t)len * sizeof(int64_t));
    }
    for (int i = 0; i < s->S; ++i) {                   // a failure on the way leaves NO shard with values
        int rc = vg_corpus_set_values(s->sh[(size_t)i], local[(size_t)i].data(), (int64_t)local[(size_t)i].size());
        if (rc != VG_OK) {
            const std::string msg = vg_last_error();
            for (auto *c : s->sh) vg_corpus_clear_values(c);
            return fail(rc, msg.c_str());
        }
    }
    return VG_OK;
}

extern "C" int vg_shards_clear_values(vg_shards *s) {
    if (!s) return fail(VG_ERR_INVALID, "shards handle is NULL");
    for (auto *c : s->sh) { int rc = vg_corpus_clear_values(c); if (rc != VG_OK) return rc; }
    return VG_OK;
}

// 1 while every shard holds values (an append drops the values of the shards it reaches)
extern "C" int vg_shards_has_values(const vg_shards *s) {
    if (!s) return 0;
    for (auto *c : s->sh) if (!vg_corpus_has_values(c)) return 0;
    return 1;
}

// ---- the fused scan forms over several shards (masked, labeled, label-set, valued, grouped, capped; the paged scans further down): every
// shard answers over its own rows, mask bits and labels through the form's _keys entry point - positions local to it - and the host
// merges the S lists of a query over GLOBAL positions.  One scaffold for all of them (point 4):
//   fused_preamble       the refusals, in one order, worded by the entry point's row of kFusedForms
//   gather_lists         keys [S][nq][pitch] (+ labels), counts [S][nq]: one call per shard, all shards in flight
//   merge_back_plain     the k best of the union by (distance image, global position) - merge_lists per query
//   merge_back_by_label  the same order, at most per_label rows of a label (grouped: one): a label can live on several shards, so
//                        the shards' rows of it compete (vg_merge_keys_capped / vg_merge_keys_grouped).  Exact: a row of the answer
//                        over all rows is in the answer of its own shard
// A single scan is a batch of one query.  A new form adds one row and one entry point whose lambda is its _keys call.
static int refuse(int code, const char *who, const char *what) {
    return fail(code, (std::string(who) + ": " + what).c_str());
}

struct FusedForm {
    const char *outer;     // whose name "NULL argument", "NULL output" and "more than 2^32 - 1 rows" carry
    const char *inner;     // ... and the nq, k, per_label, "no labels set" and "no values set" refusals
    const char *mask;      // ... and "no row mask set"; nullptr: the form reads no mask
    const char *family;    // "k must be in 1..64 (<family> scans use the fused list only)"
    bool batch, labels, by_label, capped;
    bool values;           // the valued forms: every shard must hold values
};
enum {
    F_MASKED, F_BATCH_MASKED, F_LABELED, F_BATCH_LABELED, F_LABELSET, F_BATCH_LABELSET, F_GROUPED, F_GROUPED_MASKED, F_BATCH_GROUPED,
    F_BATCH_GROUPED_MASKED, F_CAPPED, F_CAPPED_MASKED, F_BATCH_CAPPED, F_BATCH_CAPPED_MASKED, F_GROUPED_LABELSET, F_CAPPED_LABELSET,
    F_VALUED, F_VALUED_LABELED, F_BATCH_VALUED, F_GROUPED_VALUED, F_CAPPED_VALUED
};
static const FusedForm kFusedForms[] = {
    {"vg_shards_scan_topk_masked", "vg_scan_topk_masked", "vg_scan_topk_masked", "masked", false, false, false, false},
    {"vg_shards_scan_topk_batch_masked", "vg_scan_topk_batch_masked", "vg_scan_topk_batch_masked", "masked", true, false, false, false},
    {"vg_shards_scan_topk_labeled", "vg_scan_topk_labeled", nullptr, "labeled", false, true, false, false},
    {"vg_shards_scan_topk_batch_labeled", "vg_scan_topk_batch_labeled", nullptr, "labeled", true, true, false, false},
    {"vg_shards_scan_topk_labelset", "vg_scan_topk_labelset", nullptr, "label-set", false, true, false, false},
    {"vg_shards_scan_topk_batch_labelset", "vg_scan_topk_batch_labelset", nullptr, "label-set", true, true, false, false},
    {"vg_shards_scan_topk_grouped", "vg_scan_topk_grouped", nullptr, "grouped", false, true, true, false},
    {"vg_shards_scan_topk_grouped", "vg_scan_topk_grouped", "vg_scan_topk_grouped_masked", "grouped", false, true, true, false},
    {"vg_shards_scan_topk_batch_grouped", "vg_shards_scan_topk_batch_grouped", nullptr, "grouped", true, true, true, false},
    {"vg_shards_scan_topk_batch_grouped_masked", "vg_shards_scan_topk_batch_grouped_masked", "vg_shards_scan_topk_batch_grouped_masked", "grouped",
     true, true, true, false},
    {"vg_shards_scan_topk_capped", "vg_scan_topk_capped", nullptr, "capped", false, true, true, true},
    {"vg_shards_scan_topk_capped", "vg_scan_topk_capped", "vg_scan_topk_capped_masked", "capped", false, true, true, true},
    {"vg_shards_scan_topk_batch_capped", "vg_shards_scan_topk_batch_capped", nullptr, "capped", true, true, true, true},
    {"vg_shards_scan_topk_batch_capped_masked", "vg_shards_scan_topk_batch_capped_masked", "vg_shards_scan_topk_batch_capped_masked", "capped",
     true, true, true, true},
    {"vg_shards_scan_topk_grouped_labelset", "vg_shards_scan_topk_grouped_labelset", nullptr, "label-set", false, true, true, false},
    {"vg_shards_scan_topk_capped_labelset", "vg_shards_scan_topk_capped_labelset", nullptr, "label-set", false, true, true, true},
    {"vg_shards_valued_scan_topk", "vg_scan_topk_valued", nullptr, "valued", false, false, false, false, true},
    {"vg_shards_valued_scan_topk_labeled", "vg_scan_topk_valued_labeled", nullptr, "valued", false, true, false, false, true},
    {"vg_shards_valued_scan_topk_batch", "vg_scan_topk_batch_valued", nullptr, "valued", true, false, false, false, true},   // (labels: where the call names some)
    {"vg_shards_valued_scan_topk_grouped", "vg_scan_topk_grouped_valued", nullptr, "valued", false, true, true, false, true},
    {"vg_shards_valued_scan_topk_capped", "vg_scan_topk_capped_valued", nullptr, "valued", false, true, true, true, true},
};

// VG_OK: go on; FUSED_ONE_SHARD: the handle is one corpus, whose own entry point answers (and refuses); anything else: refused.
// `inputs`: the form's input pointers are all there; `outputs`: its output arrays are (the counts: out_counts, nq of them, zeroed here)
enum { FUSED_ONE_SHARD = -1 };
static int fused_preamble(int form, const vg_shards *s, int metric, bool inputs, int nq, int k, int per_label, bool outputs, int *out_counts) {
    const FusedForm &f = kFusedForms[form];
    if (!s || !inputs || !out_counts) return refuse(VG_ERR_INVALID, f.outer, "NULL argument");
    if (s->S == 1) return FUSED_ONE_SHARD;
    if (f.batch && nq < 1) return refuse(VG_ERR_INVALID, f.inner, "nq must be at least 1");
    for (int i = 0; i < nq; ++i) out_counts[i] = 0;
    if (k < 1) return refuse(VG_ERR_INVALID, f.inner, "k must be at least 1");
    if (k > VG_WAVE_KEYS) return refuse(VG_ERR_UNSUPPORTED, f.inner, (std::string("k must be in 1..64 (") + f.family + " scans use the fused list only)").c_str());
    if (f.capped && per_label < 1) return refuse(VG_ERR_INVALID, f.inner, "per_label must be at least 1");
    if (!outputs) return refuse(VG_ERR_INVALID, f.outer, "NULL output");
    if (f.mask && vg_shards_mask_count(s) < 0) return refuse(VG_ERR_INVALID, f.mask, "no row mask set");
    if (f.values && !vg_shards_has_values(s)) return refuse(VG_ERR_INVALID, f.inner, "no values set");
    if (f.labels && !vg_shards_has_labels(s)) return refuse(VG_ERR_INVALID, f.inner, "no labels set");
    if (f.by_label && s->n_rows > 0xFFFFFFFFll) return refuse(VG_ERR_UNSUPPORTED, f.outer, "more than 2^32 - 1 rows over all shards");
    // (an unknown metric stays the shards' own refusal: their entry points give it in front of some of their own argument checks - a
    //  label set's offsets, a cursor - and behind others, an order this preamble cannot reproduce for every form)
    if (vg_metric_is_bits(metric)) return vg_metric_check(s->vtype, metric, f.inner);
    return VG_OK;
}

// what the shards handed back: list (shard i, query q) at (i * nq + q) * pitch, counts[i * nq + q] of its slots valid
struct ShardLists {
    int nq = 0;
    size_t pitch = 0;
    std::vector<uint64_t> keys;
    std::vector<uint32_t> labels;
    std::vector<int> counts;
};
// scan(shard, keys, labels, counts): that shard's nq lists (labels: nullptr unless with_labels); the first failure comes back unchanged
template <typename Scan>
static int gather_lists(vg_shards *s, int nq, size_t pitch, bool with_labels, ShardLists *L, Scan scan) {
    const size_t per_shard = (size_t)nq * pitch;
    L->nq = nq;
    L->pitch = pitch;
    L->keys.assign((size_t)s->S * per_shard, VG_KEY_EMPTY);
    if (with_labels) L->labels.assign((size_t)s->S * per_shard, VG_LABEL_NONE);
    L->counts.assign((size_t)s->S * nq, 0);
    return for_each_shard(s, [&](int i) {
        return scan(i, &L->keys[(size_t)i * per_shard], with_labels ? &L->labels[(size_t)i * per_shard] : nullptr, &L->counts[(size_t)i * nq]);
    });
}

// k winners per query at out_rowids / out_dist + q * k (either may be nullptr), out_gkeys (optional): see merge_lists.  k <= 64
static int merge_back_plain(const vg_shards *s, const ShardLists &L, int k, int64_t *out_rowids, double *out_dist, uint64_t *out_gkeys,
                            int *out_counts) {
    int64_t ids[VG_WAVE_KEYS];
    double dist[VG_WAVE_KEYS];
    for (int q = 0; q < L.nq; ++q)
        out_counts[q] = merge_query_lists(s, L.keys.data(), L.counts.data(), L.nq, q, (int)L.pitch, k, out_rowids ? out_rowids + (size_t)q * k : ids,
                                          out_dist ? out_dist + (size_t)q * k : dist, -1, out_gkeys ? out_gkeys + (size_t)q * k : nullptr);
    return VG_OK;
}

// per_label >= 1: at most that many rows of a label among a query's k; otherwise the grouped form (one).  Winners at out_* + q * k
static int merge_back_by_label(const vg_shards *s, const ShardLists &L, int k, int per_label, int64_t *out_rowids, double *out_dist,
                               uint32_t *out_labels, int *out_counts) {
    const int pitch = (int)L.pitch;
    std::vector<uint64_t> qkeys((size_t)s->S * pitch), gkeys((size_t)k);
    std::vector<uint32_t> qlabels((size_t)s->S * pitch), glabels((size_t)k);
    for (int q = 0; q < L.nq; ++q) {
        for (int i = 0; i < s->S; ++i)                       // local positions -> global ones (a list stays ascending: the map is monotonic);
            for (int j = 0; j < pitch; ++j) {                // slots behind a shard's count: empty
                const size_t src = ((size_t)i * L.nq + q) * pitch + j, dst = (size_t)i * pitch + j;
                const bool held = j < L.counts[(size_t)i * L.nq + q];
                qkeys[dst] = held ? ((L.keys[src] & 0xFFFFFFFF00000000ull) | (uint64_t)global_of(s, i, (int64_t)vg_key_position(L.keys[src]))) : VG_KEY_EMPTY;
                qlabels[dst] = held ? L.labels[src] : VG_LABEL_NONE;
            }
        int cnt = 0;
        const int rc = per_label > 0 ? vg_merge_keys_capped(qkeys.data(), qlabels.data(), s->S, pitch, nullptr, k, per_label, gkeys.data(), glabels.data(), &cnt)
                                     : vg_merge_keys_grouped(qkeys.data(), qlabels.data(), s->S, pitch, nullptr, k, gkeys.data(), glabels.data(), &cnt);
        if (rc != VG_OK) return rc;
        for (int j = 0; j < cnt; ++j) {
            int shard;
            int64_t local;
            locate(s, (int64_t)vg_key_position(gkeys[(size_t)j]), &shard, &local);
            out_dist[(size_t)q * k + j] = (double)vg_key_distance(gkeys[(size_t)j]);
            out_rowids[(size_t)q * k + j] = vg_corpus_rowid_at(s->sh[(size_t)shard], local);
            out_labels[(size_t)q * k + j] = glabels[(size_t)j];
        }
        out_counts[q] = cnt;
    }
    return VG_OK;
}

extern "C" int vg_shards_scan_topk_masked(vg_shards *s, int metric, const void *query, int k, int64_t *out_rowids, double *out_dist,
                                          int *out_count) {
    int rc = fused_preamble(F_MASKED, s, metric, query, 1, k, 0, out_rowids && out_dist, out_count);
    if (rc == FUSED_ONE_SHARD) return vg_scan_topk_masked(s->sh[0], metric, query, k, out_rowids, out_dist, out_count);
    if (rc != VG_OK) return rc;
    ShardLists L;
    rc = gather_lists(s, 1, VG_WAVE_KEYS, false, &L, [&](int i, uint64_t *keys, uint32_t *, int *counts) {
        return vg_scan_topk_masked_keys(s->sh[(size_t)i], metric, query, k, keys, counts);
    });
    return rc != VG_OK ? rc : merge_back_plain(s, L, k, out_rowids, out_dist, nullptr, out_count);
}

extern "C" int vg_shards_scan_topk_batch_masked(vg_shards *s, int metric, const void *queries, int nq, int k, int64_t *out_rowids,
                                                double *out_dist, int *out_counts) {
    int rc = fused_preamble(F_BATCH_MASKED, s, metric, queries, nq, k, 0, out_rowids && out_dist, out_counts);
    if (rc == FUSED_ONE_SHARD) return vg_scan_topk_batch_masked(s->sh[0], metric, queries, nq, k, out_rowids, out_dist, out_counts);
    if (rc != VG_OK) return rc;
    ShardLists L;
    rc = gather_lists(s, nq, (size_t)k, false, &L, [&](int i, uint64_t *keys, uint32_t *, int *counts) {
        return vg_scan_topk_batch_masked_keys(s->sh[(size_t)i], metric, queries, nq, k, keys, counts);
    });
    return rc != VG_OK ? rc : merge_back_plain(s, L, k, out_rowids, out_dist, nullptr, out_counts);
}

extern "C" int vg_shards_scan_topk_labeled(vg_shards *s, int metric, const void *query, int k, uint32_t label, int64_t *out_rowids,
                                           double *out_dist, int *out_count) {
    int rc = fused_preamble(F_LABELED, s, metric, query, 1, k, 0, out_rowids && out_dist, out_count);
    if (rc == FUSED_ONE_SHARD) return vg_scan_topk_labeled(s->sh[0], metric, query, k, label, out_rowids, out_dist, out_count);
    if (rc != VG_OK) return rc;
    ShardLists L;
    rc = gather_lists(s, 1, VG_WAVE_KEYS, false, &L, [&](int i, uint64_t *keys, uint32_t *, int *counts) {
        return vg_scan_topk_labeled_keys(s->sh[(size_t)i], metric, query, k, label, keys, counts);
    });
    return rc != VG_OK ? rc : merge_back_plain(s, L, k, out_rowids, out_dist, nullptr, out_count);
}

extern "C" int vg_shards_scan_topk_batch_labeled(vg_shards *s, int metric, const void *queries, int nq, const uint32_t *query_labels, int k,
                                                 int64_t *out_rowids, double *out_dist, int *out_counts) {
    int rc = fused_preamble(F_BATCH_LABELED, s, metric, queries && query_labels, nq, k, 0, out_rowids && out_dist, out_counts);
    if (rc == FUSED_ONE_SHARD) return vg_scan_topk_batch_labeled(s->sh[0], metric, queries, nq, query_labels, k, out_rowids, out_dist, out_counts);
    if (rc != VG_OK) return rc;
    ShardLists L;
    rc = gather_lists(s, nq, (size_t)k, false, &L, [&](int i, uint64_t *keys, uint32_t *, int *counts) {
        return vg_scan_topk_batch_labeled_keys(s->sh[(size_t)i], metric, queries, nq, query_labels, k, keys, counts);
    });
    return rc != VG_OK ? rc : merge_back_plain(s, L, k, out_rowids, out_dist, nullptr, out_counts);
}

// label-set scans: a set names labels, and a label means the same on every shard - every shard gets the caller's set(s) as they are
// (and refuses a bad set itself)
extern "C" int vg_shards_scan_topk_labelset(vg_shards *s, int metric, const void *query, int k, const uint32_t *labels, int64_t n_labels,
                                            int exclude, int64_t *out_rowids, double *out_dist, int *out_count) {
    int rc = fused_preamble(F_LABELSET, s, metric, query, 1, k, 0, out_rowids && out_dist, out_count);
    if (rc == FUSED_ONE_SHARD) return vg_scan_topk_labelset(s->sh[0], metric, query, k, labels, n_labels, exclude, out_rowids, out_dist, out_count);
    if (rc != VG_OK) return rc;
    ShardLists L;
    rc = gather_lists(s, 1, VG_WAVE_KEYS, false, &L, [&](int i, uint64_t *keys, uint32_t *, int *counts) {
        return vg_scan_topk_labelset_keys(s->sh[(size_t)i], metric, query, k, labels, n_labels, exclude, keys, counts);
    });
    return rc != VG_OK ? rc : merge_back_plain(s, L, k, out_rowids, out_dist, nullptr, out_count);
}

extern "C" int vg_shards_scan_topk_batch_labelset(vg_shards *s, int metric, const void *queries, int nq, int k, const uint32_t *set_labels,
                                                  const int64_t *set_offsets, int exclude, int64_t *out_rowids, double *out_dist, int *out_counts) {
    int rc = fused_preamble(F_BATCH_LABELSET, s, metric, queries && set_offsets, nq, k, 0, out_rowids && out_dist, out_counts);
    if (rc == FUSED_ONE_SHARD)
        return vg_scan_topk_batch_labelset(s->sh[0], metric, queries, nq, k, set_labels, set_offsets, exclude, out_rowids, out_dist, out_counts);
    if (rc != VG_OK) return rc;
    ShardLists L;
    rc = gather_lists(s, nq, (size_t)k, false, &L, [&](int i, uint64_t *keys, uint32_t *, int *counts) {
        return vg_scan_topk_batch_labelset_keys(s->sh[(size_t)i], metric, queries, nq, k, set_labels, set_offsets, exclude, keys, counts);
    });
    return rc != VG_OK ? rc : merge_back_plain(s, L, k, out_rowids, out_dist, nullptr, out_counts);
}

// grouped scans: the k nearest labels, the best row of each
extern "C" int vg_shards_scan_topk_grouped(vg_shards *s, int metric, const void *query, int k, int64_t *out_rowids, double *out_dist,
                                           uint32_t *out_labels, int *out_count) {
    int rc = fused_preamble(F_GROUPED, s, metric, query, 1, k, 0, out_rowids && out_dist && out_labels, out_count);
    if (rc == FUSED_ONE_SHARD) return vg_scan_topk_grouped(s->sh[0], metric, query, k, out_rowids, out_dist, out_labels, out_count);
    if (rc != VG_OK) return rc;
    ShardLists L;
    rc = gather_lists(s, 1, VG_WAVE_KEYS, true, &L, [&](int i, uint64_t *keys, uint32_t *labels, int *counts) {
        return vg_scan_topk_grouped_keys(s->sh[(size_t)i], metric, query, k, keys, labels, counts);
    });
    return rc != VG_OK ? rc : merge_back_by_label(s, L, k, 0, out_rowids, out_dist, out_labels, out_count);
}

extern "C" int vg_shards_scan_topk_grouped_masked(vg_shards *s, int metric, const void *query, int k, int64_t *out_rowids, double *out_dist,
                                                  uint32_t *out_labels, int *out_count) {
    int rc = fused_preamble(F_GROUPED_MASKED, s, metric, query, 1, k, 0, out_rowids && out_dist && out_labels, out_count);
    if (rc == FUSED_ONE_SHARD) return vg_scan_topk_grouped_masked(s->sh[0], metric, query, k, out_rowids, out_dist, out_labels, out_count);
    if (rc != VG_OK) return rc;
    ShardLists L;
    rc = gather_lists(s, 1, VG_WAVE_KEYS, true, &L, [&](int i, uint64_t *keys, uint32_t *labels, int *counts) {
        return vg_scan_topk_grouped_masked_keys(s->sh[(size_t)i], metric, query, k, keys, labels, counts);
    });
    return rc != VG_OK ? rc : merge_back_by_label(s, L, k, 0, out_rowids, out_dist, out_labels, out_count);
}

extern "C" int vg_shards_scan_topk_batch_grouped(vg_shards *s, int metric, const void *queries, int nq, int k, int64_t *out_rowids,
                                                 double *out_dist, uint32_t *out_labels, int *out_counts) {
    int rc = fused_preamble(F_BATCH_GROUPED, s, metric, queries, nq, k, 0, out_rowids && out_dist && out_labels, out_counts);
    if (rc == FUSED_ONE_SHARD) return vg_scan_topk_batch_grouped(s->sh[0], metric, queries, nq, k, out_rowids, out_dist, out_labels, out_counts);
    if (rc != VG_OK) return rc;
    ShardLists L;
    rc = gather_lists(s, nq, (size_t)k, true, &L, [&](int i, uint64_t *keys, uint32_t *labels, int *counts) {
        return vg_scan_topk_batch_grouped_keys(s->sh[(size_t)i], metric, queries, nq, k, keys, labels, counts);
    });
    return rc != VG_OK ? rc : merge_back_by_label(s, L, k, 0, out_rowids, out_dist, out_labels, out_counts);
}

extern "C" int vg_shards_scan_topk_batch_grouped_masked(vg_shards *s, int metric, const void *queries, int nq, int k, int64_t *out_rowids,
                                                        double *out_dist, uint32_t *out_labels, int *out_counts) {
    int rc = fused_preamble(F_BATCH_GROUPED_MASKED, s, metric, queries, nq, k, 0, out_rowids && out_dist && out_labels, out_counts);
    if (rc == FUSED_ONE_SHARD) return vg_scan_topk_batch_grouped_masked(s->sh[0], metric, queries, nq, k, out_rowids, out_dist, out_labels, out_counts);
    if (rc != VG_OK) return rc;
    ShardLists L;
    rc = gather_lists(s, nq, (size_t)k, true, &L, [&](int i, uint64_t *keys, uint32_t *labels, int *counts) {
        return vg_scan_topk_batch_grouped_masked_keys(s->sh[(size_t)i], metric, queries, nq, k, keys, labels, counts);
    });
    return rc != VG_OK ? rc : merge_back_by_label(s, L, k, 0, out_rowids, out_dist, out_labels, out_counts);
}

// capped scans: the k nearest rows, at most per_label of one label
extern "C" int vg_shards_scan_topk_capped(vg_shards *s, int metric, const void *query, int k, int per_label, int64_t *out_rowids,
                                          double *out_dist, uint32_t *out_labels, int *out_count) {
    int rc = fused_preamble(F_CAPPED, s, metric, query, 1, k, per_label, out_rowids && out_dist && out_labels, out_count);
    if (rc == FUSED_ONE_SHARD) return vg_scan_topk_capped(s->sh[0], metric, query, k, per_label, out_rowids, out_dist, out_labels, out_count);
    if (rc != VG_OK) return rc;
    ShardLists L;
    rc = gather_lists(s, 1, VG_WAVE_KEYS, true, &L, [&](int i, uint64_t *keys, uint32_t *labels, int *counts) {
        return vg_scan_topk_capped_keys(s->sh[(size_t)i], metric, query, k, per_label, keys, labels, counts);
    });
    return rc != VG_OK ? rc : merge_back_by_label(s, L, k, per_label, out_rowids, out_dist, out_labels, out_count);
}

extern "C" int vg_shards_scan_topk_capped_masked(vg_shards *s, int metric, const void *query, int k, int per_label, int64_t *out_rowids,
                                                 double *out_dist, uint32_t *out_labels, int *out_count) {
    int rc = fused_preamble(F_CAPPED_MASKED, s, metric, query, 1, k, per_label, out_rowids && out_dist && out_labels, out_count);
    if (rc == FUSED_ONE_SHARD) return vg_scan_topk_capped_masked(s->sh[0], metric, query, k, per_label, out_rowids, out_dist, out_labels, out_count);
    if (rc != VG_OK) return rc;
    ShardLists L;
    rc = gather_lists(s, 1, VG_WAVE_KEYS, true, &L, [&](int i, uint64_t *keys, uint32_t *labels, int *counts) {
        return vg_scan_topk_capped_masked_keys(s->sh[(size_t)i], metric, query, k, per_label, keys, labels, counts);
    });
    return rc != VG_OK ? rc : merge_back_by_label(s, L, k, per_label, out_rowids, out_dist, out_labels, out_count);
}

extern "C" int vg_shards_scan_topk_batch_capped(vg_shards *s, int metric, const void *queries, int nq, int k, int per_label, int64_t *out_rowids,
                                                double *out_dist, uint32_t *out_labels, int *out_counts) {
    int rc = fused_preamble(F_BATCH_CAPPED, s, metric, queries, nq, k, per_label, out_rowids && out_dist && out_labels, out_counts);
    if (rc == FUSED_ONE_SHARD)
        return vg_scan_topk_batch_capped(s->sh[0], metric, queries, nq, k, per_label, out_rowids, out_dist, out_labels, out_counts);
    if (rc != VG_OK) return rc;
    ShardLists L;
    rc = gather_lists(s, nq, (size_t)k, true, &L, [&](int i, uint64_t *keys, uint32_t *labels, int *counts) {
        return vg_scan_topk_batch_capped_keys(s->sh[(size_t)i], metric, queries, nq, k, per_label, keys, labels, counts);
    });
    return rc != VG_OK ? rc : merge_back_by_label(s, L, k, per_label, out_rowids, out_dist, out_labels, out_counts);
}

extern "C" int vg_shards_scan_topk_batch_capped_masked(vg_shards *s, int metric, const void *queries, int nq, int k, int per_label, int64_t *out_rowids,
                                                       double *out_dist, uint32_t *out_labels, int *out_counts) {
    int rc = fused_preamble(F_BATCH_CAPPED_MASKED, s, metric, queries, nq, k, per_label, out_rowids && out_dist && out_labels, out_counts);
    if (rc == FUSED_ONE_SHARD)
        return vg_scan_topk_batch_capped_masked(s->sh[0], metric, queries, nq, k, per_label, out_rowids, out_dist, out_labels, out_counts);
    if (rc != VG_OK) return rc;
    ShardLists L;
    rc = gather_lists(s, nq, (size_t)k, true, &L, [&](int i, uint64_t *keys, uint32_t *labels, int *counts) {
        return vg_scan_topk_batch_capped_masked_keys(s->sh[(size_t)i], metric, queries, nq, k, per_label, keys, labels, counts);
    });
    return rc != VG_OK ? rc : merge_back_by_label(s, L, k, per_label, out_rowids, out_dist, out_labels, out_counts);
}

extern "C" int vg_shards_scan_topk_grouped_labelset(vg_shards *s, int metric, const void *query, int k, const uint32_t *labels, int64_t n_labels,
                                                    int exclude, int64_t *out_rowids, double *out_dist, uint32_t *out_labels, int *out_count) {
    int rc = fused_preamble(F_GROUPED_LABELSET, s, metric, query, 1, k, 0, out_rowids && out_dist && out_labels, out_count);
    if (rc == FUSED_ONE_SHARD)
        return vg_scan_topk_grouped_labelset(s->sh[0], metric, query, k, labels, n_labels, exclude, out_rowids, out_dist, out_labels, out_count);
    if (rc != VG_OK) return rc;
    ShardLists L;
    rc = gather_lists(s, 1, VG_WAVE_KEYS, true, &L, [&](int i, uint64_t *keys, uint32_t *klabels, int *counts) {
        return vg_scan_topk_grouped_labelset_keys(s->sh[(size_t)i], metric, query, k, labels, n_labels, exclude, keys, klabels, counts);
    });
    return rc != VG_OK ? rc : merge_back_by_label(s, L, k, 0, out_rowids, out_dist, out_labels, out_count);
}

extern "C" int vg_shards_scan_topk_capped_labelset(vg_shards *s, int metric, const void *query, int k, int per_label, const uint32_t *labels,
                                                   int64_t n_labels, int exclude, int64_t *out_rowids, double *out_dist, uint32_t *out_labels,
                                                   int *out_count) {
    if (out_count) *out_count = 0;
    if (per_label < 1) return fail(VG_ERR_INVALID, "vg_shards_scan_topk_capped_labelset: per_label must be at least 1");
    int rc = fused_preamble(F_CAPPED_LABELSET, s, metric, query, 1, k, per_label, out_rowids && out_dist && out_labels, out_count);
    if (rc == FUSED_ONE_SHARD)
        return vg_scan_topk_capped_labelset(s->sh[0], metric, query, k, per_label, labels, n_labels, exclude, out_rowids, out_dist, out_labels, out_count);
    if (rc != VG_OK) return rc;
    ShardLists L;
    rc = gather_lists(s, 1, VG_WAVE_KEYS, true, &L, [&](int i, uint64_t *keys, uint32_t *klabels, int *counts) {
        return vg_scan_topk_capped_labelset_keys(s->sh[(size_t)i], metric, query, k, per_label, labels, n_labels, exclude, keys, klabels, counts);
    });
    return rc != VG_OK ? rc : merge_back_by_label(s, L, k, per_label, out_rowids, out_dist, out_labels, out_count);
}

// value-range scans: an interval means the same on every shard - every shard gets the caller's interval(s), and labels, as they are
extern "C" int vg_shards_valued_scan_topk(vg_shards *s, int metric, const void *query, int k, int64_t lo, int64_t hi, int64_t *out_rowids,
                                          double *out_dist, int *out_count) {
    int rc = fused_preamble(F_VALUED, s, metric, query, 1, k, 0, out_rowids && out_dist, out_count);
    if (rc == FUSED_ONE_SHARD) return vg_scan_topk_valued(s->sh[0], metric, query, k, lo, hi, out_rowids, out_dist, out_count);
    if (rc != VG_OK) return rc;
    ShardLists L;
    rc = gather_lists(s, 1, VG_WAVE_KEYS, false, &L, [&](int i, uint64_t *keys, uint32_t *, int *counts) {
        return vg_scan_topk_valued_keys(s->sh[(size_t)i], metric, query, k, lo, hi, keys, counts);
    });
    return rc != VG_OK ? rc : merge_back_plain(s, L, k, out_rowids, out_dist, nullptr, out_count);
}

extern "C" int vg_shards_valued_scan_topk_labeled(vg_shards *s, int metric, const void *query, int k, int64_t lo, int64_t hi, uint32_t label,
                                                  int64_t *out_rowids, double *out_dist, int *out_count) {
    int rc = fused_preamble(F_VALUED_LABELED, s, metric, query, 1, k, 0, out_rowids && out_dist, out_count);
    if (rc == FUSED_ONE_SHARD) return vg_scan_topk_valued_labeled(s->sh[0], metric, query, k, lo, hi, label, out_rowids, out_dist, out_count);
    if (rc != VG_OK) return rc;
    ShardLists L;
    rc = gather_lists(s, 1, VG_WAVE_KEYS, false, &L, [&](int i, uint64_t *keys, uint32_t *, int *counts) {
        return vg_scan_topk_valued_labeled_keys(s->sh[(size_t)i], metric, query, k, lo, hi, label, keys, counts);
    });
    return rc != VG_OK ? rc : merge_back_plain(s, L, k, out_rowids, out_dist, nullptr, out_count);
}

extern "C" int vg_shards_valued_scan_topk_batch(vg_shards *s, int metric, const void *queries, int nq, int k, const int64_t *los,
                                                const int64_t *his, const uint32_t *query_labels, int64_t *out_rowids, double *out_dist,
                                                int *out_counts) {
    int rc = fused_preamble(F_BATCH_VALUED, s, metric, queries && los && his, nq, k, 0, out_rowids && out_dist, out_counts);
    if (rc == FUSED_ONE_SHARD)
        return vg_scan_topk_batch_valued(s->sh[0], metric, queries, nq, k, los, his, query_labels, out_rowids, out_dist, out_counts);
    if (rc != VG_OK) return rc;
    if (query_labels && !vg_shards_has_labels(s)) return refuse(VG_ERR_INVALID, kFusedForms[F_BATCH_VALUED].inner, "no labels set");
    ShardLists L;
    rc = gather_lists(s, nq, (size_t)k, false, &L, [&](int i, uint64_t *keys, uint32_t *, int *counts) {
        return vg_scan_topk_batch_valued_keys(s->sh[(size_t)i], metric, queries, nq, k, los, his, query_labels, keys, counts);
    });
    return rc != VG_OK ? rc : merge_back_plain(s, L, k, out_rowids, out_dist, nullptr, out_counts);
}

extern "C" int vg_shards_valued_scan_topk_grouped(vg_shards *s, int metric, const void *query, int k, int64_t lo, int64_t hi,
                                                  int64_t *out_rowids, double *out_dist, uint32_t *out_labels, int *out_count) {
    int rc = fused_preamble(F_GROUPED_VALUED, s, metric, query, 1, k, 0, out_rowids && out_dist && out_labels, out_count);
    if (rc == FUSED_ONE_SHARD) return vg_scan_topk_grouped_valued(s->sh[0], metric, query, k, lo, hi, out_rowids, out_dist, out_labels, out_count);
    if (rc != VG_OK) return rc;
    ShardLists L;
    rc = gather_lists(s, 1, VG_WAVE_KEYS, true, &L, [&](int i, uint64_t *keys, uint32_t *klabels, int *counts) {
        return vg_scan_topk_grouped_valued_keys(s->sh[(size_t)i], metric, query, k, lo, hi, keys, klabels, counts);
    });
    return rc != VG_OK ? rc : merge_back_by_label(s, L, k, 0, out_rowids, out_dist, out_labels, out_count);
}

extern "C" int vg_shards_valued_scan_topk_capped(vg_shards *s, int metric, const void *query, int k, int per_label, int64_t lo, int64_t hi,
                                                 int64_t *out_rowids, double *out_dist, uint32_t *out_labels, int *out_count) {
    if (out_count) *out_count = 0;
    if (per_label < 1) return fail(VG_ERR_INVALID, "vg_shards_valued_scan_topk_capped: per_label must be at least 1");
    int rc = fused_preamble(F_CAPPED_VALUED, s, metric, query, 1, k, per_label, out_rowids && out_dist && out_labels, out_count);
    if (rc == FUSED_ONE_SHARD)
        return vg_scan_topk_capped_valued(s->sh[0], metric, query, k, per_label, lo, hi, out_rowids, out_dist, out_labels, out_count);
    if (rc != VG_OK) return rc;
    ShardLists L;
    rc = gather_lists(s, 1, VG_WAVE_KEYS, true, &L, [&](int i, uint64_t *keys, uint32_t *klabels, int *counts) {
        return vg_scan_topk_capped_valued_keys(s->sh[(size_t)i], metric, query, k, per_label, lo, hi, keys, klabels, counts);
    });
    return rc != VG_OK ? rc : merge_back_by_label(s, L, k, per_label, out_rowids, out_dist, out_labels, out_count);
}

// ---- paged scans (vg_scan_after.hip, vg_multi_after.hip): a cursor over GLOBAL scan order becomes one floor key per shard over ITS
// positions - the cursor's distance image with "local rows of this shard in front of global position P" (local_rows_before) - every
// shard runs its floor form and the lists merge like the masked scans', by (distance image, global position)
struct AfterWho { const char *one, *batch; };
static AfterWho after_who(bool masked) {
    return masked ? AfterWho{"vg_scan_topk_after_masked", "vg_scan_topk_batch_after_masked"} : AfterWho{"vg_scan_topk_after", "vg_scan_topk_batch_after"};
}
// floors[i] for a (distance, rowid) cursor; every shard's rowids must be ascending (the rows are dealt out in global order)
static int shard_floors_cursor(const vg_shards *s, const char *who, double after_dist, int64_t after_rowid, uint64_t *floors) {
    if (after_dist != after_dist) return refuse(VG_ERR_INVALID, who, "the cursor's distance is NaN");
    int64_t P = 0;
    for (auto *c : s->sh) {
        const int64_t p = vg_corpus_rows_upto_rowid(c, after_rowid);
        if (p == -2) return refuse(VG_ERR_UNSUPPORTED, who, "the rowids are not ascending (no rowid order); page by key (the _keys form)");
        P += p;
    }
    // ascending inside every shard is not ascending in GLOBAL order: blocks are dealt out cyclically, so every block border is
    // compared too (n_rows / B lookups) - one corpus holding these rows would refuse them, and so do the shards
    for (int64_t g = s->B; g < s->n_rows; g += s->B)
        if (vg_shards_rowid_at(s, g - 1) >= vg_shards_rowid_at(s, g))
            return refuse(VG_ERR_UNSUPPORTED, who, "the rowids are not ascending in global order (no rowid order); page by key (the _keys form)");
    for (int i = 0; i < s->S; ++i) {
        int empty = 0;
        const int64_t local = std::min<int64_t>(local_rows_before(s, i, P), vg_corpus_rows(s->sh[(size_t)i]));
        int rc = vg_after_floor(after_dist, (uint32_t)local, &floors[i], &empty);      // (empty: VG_KEY_EMPTY, no launch)
        if (rc != VG_OK) return rc;
    }
    return VG_OK;
}
// floors[i] for a cursor given as the last GLOBAL key of the previous page
static int shard_floors_key(const vg_shards *s, const char *who, uint64_t after_key, uint64_t *floors) {
    if (after_key == VG_KEY_EMPTY) return refuse(VG_ERR_INVALID, who, "after_key is the empty key");
    if (s->n_rows >= (1ll << 32)) return refuse(VG_ERR_UNSUPPORTED, who, "keys over global positions need fewer than 2^32 rows");
    const uint64_t g = after_key + 1ull;
    for (int i = 0; i < s->S; ++i) {
        const int64_t local = std::min<int64_t>(local_rows_before(s, i, (int64_t)(g & 0xFFFFFFFFull)), vg_corpus_rows(s->sh[(size_t)i]));
        floors[i] = (g & 0xFFFFFFFF00000000ull) | (uint64_t)local;
    }
    return VG_OK;
}

// one query, the floors of the S shards given; out_gkeys (keys form) or out_rowids / out_dist
static int shards_after_run(vg_shards *s, bool masked, int metric, const void *query, int k, const uint64_t *floors, int64_t *out_rowids,
                            double *out_dist, uint64_t *out_gkeys, int *out_count) {
    const char *who = after_who(masked).one;
    if (k < 1) return refuse(VG_ERR_INVALID, who, "k must be at least 1");
    if (k > VG_WAVE_KEYS) return refuse(VG_ERR_UNSUPPORTED, who, "k must be in 1..64 (paged scans use the fused list only)");
    if (masked && vg_shards_mask_count(s) < 0) return refuse(VG_ERR_INVALID, who, "no row mask set");
    ShardLists L;
    const int rc = gather_lists(s, 1, VG_WAVE_KEYS, false, &L, [&](int i, uint64_t *keys, uint32_t *, int *counts) {
        return vg_after_floor_run(s->sh[(size_t)i], masked, metric, query, k, floors[i], keys, counts);
    });
    return rc != VG_OK ? rc : merge_back_plain(s, L, k, out_rowids, out_dist, out_gkeys, out_count);
}

static int shards_after(vg_shards *s, bool masked, int metric, const void *query, int k, double after_dist, int64_t after_rowid,
                        int64_t *out_rowids, double *out_dist, int *out_count) {
    const char *who = after_who(masked).one;
    if (!s || !query || !out_count) return refuse(VG_ERR_INVALID, who, "NULL argument");
    if (s->S == 1) return masked ? vg_scan_topk_after_masked(s->sh[0], metric, query, k, after_dist, after_rowid, out_rowids, out_dist, out_count)
                                 : vg_scan_topk_after(s->sh[0], metric, query, k, after_dist, after_rowid, out_rowids, out_dist, out_count);
    *out_count = 0;
    if (k >= 1 && k <= VG_WAVE_KEYS && (!out_rowids || !out_dist)) return refuse(VG_ERR_INVALID, who, "NULL output");
    std::vector<uint64_t> floors((size_t)s->S, VG_KEY_EMPTY);
    int rc = shard_floors_cursor(s, who, after_dist, after_rowid, floors.data());
    if (rc != VG_OK) return rc;
    return shards_after_run(s, masked, metric, query, k, floors.data(), out_rowids, out_dist, nullptr, out_count);
}
static int shards_after_keys(vg_shards *s, bool masked, int metric, const void *query, int k, uint64_t after_key, uint64_t *out_keys, int *out_count) {
    const char *who = after_who(masked).one;
    if (!s || !query || !out_count) return refuse(VG_ERR_INVALID, who, "NULL argument");
    if (s->S == 1) return masked ? vg_scan_topk_after_masked_keys(s->sh[0], metric, query, k, after_key, out_keys, out_count)
                                 : vg_scan_topk_after_keys(s->sh[0], metric, query, k, after_key, out_keys, out_count);
    *out_count = 0;
    if (k >= 1 && k <= VG_WAVE_KEYS && !out_keys) return refuse(VG_ERR_INVALID, who, "NULL output");
    std::vector<uint64_t> floors((size_t)s->S, VG_KEY_EMPTY);
    int rc = shard_floors_key(s, who, after_key, floors.data());
    if (rc != VG_OK) return rc;
    return shards_after_run(s, masked, metric, query, k, floors.data(), nullptr, nullptr, out_keys, out_count);
}

// the batch: floors [S][nq]; every shard answers all nq queries behind its own floors, then one merge per query
static int shards_after_batch_run(vg_shards *s, bool masked, int metric, const void *queries, int nq, int k, const uint64_t *floors,
                                  int64_t *out_rowids, double *out_dist, uint64_t *out_gkeys, int *out_counts) {
    const char *who = after_who(masked).batch;
    if (k < 1) return refuse(VG_ERR_INVALID, who, "k must be at least 1");
    if (k > VG_WAVE_KEYS) return refuse(VG_ERR_UNSUPPORTED, who, "k must be in 1..64 (paged scans use the fused list only)");
    if (masked && vg_shards_mask_count(s) < 0) return refuse(VG_ERR_INVALID, who, "no row mask set");
    ShardLists L;
    const int rc = gather_lists(s, nq, (size_t)k, false, &L, [&](int i, uint64_t *keys, uint32_t *, int *counts) {
        return vg_after_floor_batch_run(s->sh[(size_t)i], masked, metric, queries, nq, k, floors + (size_t)i * nq, keys, counts);
    });
    return rc != VG_OK ? rc : merge_back_plain(s, L, k, out_rowids, out_dist, out_gkeys, out_counts);
}

static int shards_after_batch(vg_shards *s, bool masked, int metric, const void *queries, int nq, int k, const double *after_dists,
                              const int64_t *after_rowids, int64_t *out_rowids, double *out_dist, int *out_counts) {
    const char *who = after_who(masked).batch;
    if (!s || !queries || !out_counts || !after_dists || !after_rowids) return refuse(VG_ERR_INVALID, who, "NULL argument");
    if (s->S == 1) return masked ? vg_scan_topk_batch_after_masked(s->sh[0], metric, queries, nq, k, after_dists, after_rowids, out_rowids, out_dist, out_counts)
                                 : vg_scan_topk_batch_after(s->sh[0], metric, queries, nq, k, after_dists, after_rowids, out_rowids, out_dist, out_counts);
    if (nq < 1) return refuse(VG_ERR_INVALID, who, "nq must be at least 1");
    for (int i = 0; i < nq; ++i) out_counts[i] = 0;
    if (k >= 1 && k <= VG_WAVE_KEYS && (!out_rowids || !out_dist)) return refuse(VG_ERR_INVALID, who, "NULL output");
    std::vector<uint64_t> floors((size_t)s->S * nq, VG_KEY_EMPTY), one((size_t)s->S);
    for (int q = 0; q < nq; ++q) {
        int rc = shard_floors_cursor(s, who, after_dists[q], after_rowids[q], one.data());
        if (rc != VG_OK) return rc;
        for (int i = 0; i < s->S; ++i) floors[(size_t)i * nq + q] = one[(size_t)i];
    }
    return shards_after_batch_run(s, masked, metric, queries, nq, k, floors.data(), out_rowids, out_dist, nullptr, out_counts);
}
static int shards_after_batch_keys(vg_shards *s, bool masked, int metric, const void *queries, int nq, int k, const uint64_t *after_keys,
                                   uint64_t *out_keys, int *out_counts) {
    const char *who = after_who(masked).batch;
    if (!s || !queries || !out_counts || !after_keys) return refuse(VG_ERR_INVALID, who, "NULL argument");
    if (s->S == 1) return masked ? vg_scan_topk_batch_after_masked_keys(s->sh[0], metric, queries, nq, k, after_keys, out_keys, out_counts)
                                 : vg_scan_topk_batch_after_keys(s->sh[0], metric, queries, nq, k, after_keys, out_keys, out_counts);
    if (nq < 1) return refuse(VG_ERR_INVALID, who, "nq must be at least 1");
    for (int i = 0; i < nq; ++i) out_counts[i] = 0;
    if (k >= 1 && k <= VG_WAVE_KEYS && !out_keys) return refuse(VG_ERR_INVALID, who, "NULL output");
    std::vector<uint64_t> floors((size_t)s->S * nq, VG_KEY_EMPTY), one((size_t)s->S);
    for (int q = 0; q < nq; ++q) {
        int rc = shard_floors_key(s, who, after_keys[q], one.data());
        if (rc != VG_OK) return rc;
        for (int i = 0; i < s->S; ++i) floors[(size_t)i * nq + q] = one[(size_t)i];
    }
    return shards_after_batch_run(s, masked, metric, queries, nq, k, floors.data(), nullptr, nullptr, out_keys, out_counts);
}

extern "C" int vg_shards_scan_topk_after(vg_shards *s, int metric, const void *query, int k, double after_dist, int64_t after_rowid,
                                         int64_t *out_rowids, double *out_dist, int *out_count) {
    return shards_after(s, false, metric, query, k, after_dist, after_rowid, out_rowids, out_dist, out_count);
}
extern "C" int vg_shards_scan_topk_after_keys(vg_shards *s, int metric, const void *query, int k, uint64_t after_key, uint64_t *out_keys,
                                              int *out_count) {
    return shards_after_keys(s, false, metric, query, k, after_key, out_keys, out_count);
}
extern "C" int vg_shards_scan_topk_after_masked(vg_shards *s, int metric, const void *query, int k, double after_dist, int64_t after_rowid,
                                                int64_t *out_rowids, double *out_dist, int *out_count) {
    return shards_after(s, true, metric, query, k, after_dist, after_rowid, out_rowids, out_dist, out_count);
}
extern "C" int vg_shards_scan_topk_after_masked_keys(vg_shards *s, int metric, const void *query, int k, uint64_t after_key,
                                                     uint64_t *out_keys, int *out_count) {
    return shards_after_keys(s, true, metric, query, k, after_key, out_keys, out_count);
}
extern "C" int vg_shards_scan_topk_batch_after(vg_shards *s, int metric, const void *queries, int nq, int k, const double *after_dists,
                                               const int64_t *after_rowids, int64_t *out_rowids, double *out_dist, int *out_counts) {
    return shards_after_batch(s, false, metric, queries, nq, k, after_dists, after_rowids, out_rowids, out_dist, out_counts);
}
extern "C" int vg_shards_scan_topk_batch_after_keys(vg_shards *s, int metric, const void *queries, int nq, int k, const uint64_t *after_keys,
                                                    uint64_t *out_keys, int *out_counts) {
    return shards_after_batch_keys(s, false, metric, queries, nq, k, after_keys, out_keys, out_counts);
}
extern "C" int vg_shards_scan_topk_batch_after_masked(vg_shards *s, int metric, const void *queries, int nq, int k, const double *after_dists,
                                                      const int64_t *after_rowids, int64_t *out_rowids, double *out_dist, int *out_counts) {
    return shards_after_batch(s, true, metric, queries, nq, k, after_dists, after_rowids, out_rowids, out_dist, out_counts);
}
extern "C" int vg_shards_scan_topk_batch_after_masked_keys(vg_shards *s, int metric, const void *queries, int nq, int k,
                                                           const uint64_t *after_keys, uint64_t *out_keys, int *out_counts) {
    return shards_after_batch_keys(s, true, metric, queries, nq, k, after_keys, out_keys, out_counts);
}

extern "C" int vg_shards_minmax(vg_shards *s, float *out_min, float *out_max, int *out_any_negative) {
    if (!s || !out_min || !out_max || !out_any_negative) return fail(VG_ERR_INVALID, "vg_shards_minmax: NULL argument");
    if (s->S == 1) return vg_corpus_minmax(s->sh[0], out_min, out_max, out_any_negative);
    std::vector<float> lo((size_t)s->S), hi((size_t)s->S);
    std::vector<int> neg((size_t)s->S);
    int rc = for_each_shard(s, [&](int i) { return vg_corpus_minmax(s->sh[(size_t)i], &lo[(size_t)i], &hi[(size_t)i], &neg[(size_t)i]); });
    if (rc != VG_OK) return rc;
    *out_min = lo[0]; *out_max = hi[0]; *out_any_negative = neg[0];
    for (int i = 1; i < s->S; ++i) {
        if (lo[(size_t)i] < *out_min) *out_min = lo[(size_t)i];
        if (hi[(size_t)i] > *out_max) *out_max = hi[(size_t)i];
        *out_any_negative |= neg[(size_t)i];
    }
    return VG_OK;
}

extern "C" int vg_shards_quantize_rows(vg_shards *s, float scale, float offset, int qtype, int64_t row0, int64_t n_rows,
                                       uint8_t *out_host) {
    if (!s || !out_host) return fail(VG_ERR_INVALID, "vg_shards_quantize_rows: NULL argument");
    if (s->S == 1) return vg_corpus_quantize_rows(s->sh[0], scale, offset, qtype, row0, n_rows, out_host);
    if (row0 < 0 || n_rows < 0 || row0 + n_rows > s->n_rows) return fail(VG_ERR_INVALID, "vg_shards_quantize_rows: row range out of bounds");
    int64_t g = row0;
    while (g < row0 + n_rows) {
        int shard;
        int64_t local;
        locate(s, g, &shard, &local);
        const int64_t take = std::min<int64_t>(s->B - g % s->B, row0 + n_rows - g);
        int rc = vg_corpus_quantize_rows(s->sh[(size_t)shard], scale, offset, qtype, local, take, out_host + (g - row0) * s->dim);
        if (rc != VG_OK) return rc;
        g += take;
    }
    return VG_OK;
}
