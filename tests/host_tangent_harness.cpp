// CPU harness of the host half of the rebuilt tangent (csrc/fcamd_hosttangent.cpp): the pool of expansion threads, the three expanders
// and the chunk plan, driven by a producer that plays the device's part of run_param_chunks' protocol (csrc/fcamd_hostpath.cpp).  No GPU:
// the seven HIP calls the file needs are stubs (the ring is plain heap memory of exactly the size host_tangent_ring asks for, so that
// AddressSanitizer sees a write past it).  Built by tests/test_host_tangent_pool.py plain, with ThreadSanitizer and with ASan + UBSan.
//
//   harness plan  N OPT_CHUNK PRM                       -> "chunk nslots slot_doubles nchunks start[0] .. start[nchunks]"
//   harness plans                                       -> the same for every "N OPT_CHUNK PRM" line of the standard input
//   harness parts NP THREADS KIND                       -> one line per task of ExpandPool::post(0, NP, src, mask): "a b src_doubles mask_words"
//   harness run   KIND TD N THREADS NSLOTS MODE OFF DIR -> DIR/tangent.f64 (canary margin, td * N doubles, canary margin)
//
// KIND: 0 CONST, 1 MISES, 2 MISES_COMFE, 3 DRUCKER_PRAGER (HostTangentJob::Kind).  MODE 0: the calling thread fills a slot and posts it;
// MODE 1: a second thread fills the slots and publishes them through an atomic, the calling thread picks them up as hipEventQuery /
// hipEventSynchronize would.  OFF: elements the tangent starts behind a 16-byte boundary (0 or 1: the two store paths).
// DIR holds tables.f64 (Tables::a, ::b, ::c, then Scalars::s[16]), params.f64 (PRM doubles for EVERY point; only those of plastic points
// are copied into the ring), ballots.u64 (one word per 64 points of the call) and starts.i64 (the chunk starts, the last one N).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <limits>
#include <string>
#include <thread>
#include <vector>

#include "fcamd_host.h"

// ---- what the library's other translation units and the HIP runtime would supply ------------------------------------------------
namespace fcamd {
int fail(int status, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
    return status;
}
}  // namespace fcamd

extern "C" {
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) {
    *e = reinterpret_cast<hipEvent_t>(new int(0));
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) {
    delete reinterpret_cast<int*>(e);
    return hipSuccess;
}
const char* hipGetErrorString(hipError_t) { return "stub"; }
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipHostFree(void* p) {
    free(p);
    return hipSuccess;
}
hipError_t hipHostGetDevicePointer(void** d, void* h, unsigned) {
    *d = h;
    return hipSuccess;
}
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) {
    *p = malloc(bytes);
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
}

// the pool's task queue is private; the `parts` command reads it (every standard header the file includes has been included above)
#define private public
#include "fcamd_hosttangent.cpp"
#undef private

using namespace fcamd;

namespace {

constexpr int64_t kMargin = 256;                  // canary doubles on either side of the tangent
constexpr unsigned long long kCanary = 0x7ff4c0dec0dec0deull;  // (a NaN no arithmetic produces)

template <class T>
std::vector<T> read_file(const std::string& path) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path.c_str());
        exit(2);
    }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<T> v((size_t)bytes / sizeof(T));
    if (!v.empty() && fread(v.data(), sizeof(T), v.size(), f) != v.size()) exit(2);
    fclose(f);
    return v;
}

void print_plan(long long n, long long opt, int prm) {
    const HostTangentPlan p = host_tangent_plan(n, opt, prm);
    printf("%lld %d %zu %zu", (long long)p.chunk, p.nslots, host_tangent_slot_doubles(p.chunk, prm), p.start.size() - 1);
    for (int64_t s : p.start) printf(" %lld", (long long)s);
    printf("\n");
}

int cmd_plan(char** a) {
    print_plan(atoll(a[0]), atoll(a[1]), atoi(a[2]));
    return 0;
}

int cmd_plans() {  // "N OPT_CHUNK PRM" per line of the standard input
    long long n, opt;
    int prm;
    while (scanf("%lld %lld %d", &n, &opt, &prm) == 3) print_plan(n, opt, prm);
    return 0;
}

int cmd_parts(char** a) {
    const int64_t np = atoll(a[0]);
    const int threads = atoi(a[1]);
    const int kind = atoi(a[2]);
    ExpandPool pool(0);
    pool.workers_.resize((size_t)threads);  // threads() == threads, nobody takes the tasks
    HostTangentJob job{};
    job.kind = (HostTangentJob::Kind)kind;
    job.prm = kind == HostTangentJob::DRUCKER_PRAGER ? 12 : 8;
    job.td = 36;
    pool.begin(job);
    static const double src[1] = {0.0};
    static const unsigned long long mask[1] = {0ull};
    const int ticket = pool.post(0, np, kind == HostTangentJob::CONST ? nullptr : src, kind == HostTangentJob::CONST ? nullptr : mask);
    pool.workers_.clear();
    if ((int)pool.tasks_.size() != pool.left_[(size_t)ticket]) return 3;
    for (const auto& t : pool.tasks_)
        printf("%lld %lld %lld %lld\n", (long long)t.p0, (long long)t.p1, t.src ? (long long)(t.src - src) : -1ll, t.mask ? (long long)(t.mask - mask) : -1ll);
    pool.tasks_.clear();
    return 0;
}

int cmd_run(char** a) {
    const int kind = atoi(a[0]), td = atoi(a[1]);
    const int64_t n = atoll(a[2]);
    const int threads = atoi(a[3]), nslots = atoi(a[4]), mode = atoi(a[5]), off = atoi(a[6]);
    const std::string dir = a[7];
    const std::vector<double> tables = read_file<double>(dir + "/tables.f64");
    if (tables.size() != 3 * 36 + 16) return 2;

    fcamd_context* c = new fcamd_context;
    c->opt.host_tangent_threads = threads;
    fcamd_model* m = new fcamd_model;
    m->ctx = c;
    const int laws[4] = {FCAMD_LINEAR_ELASTICITY, FCAMD_VON_MISES_3D, FCAMD_COMFE_MISES_PLASTICITY, FCAMD_COMFE_DRUCKER_PRAGER};
    m->law = laws[kind];
    m->dims.sd = td == 36 ? 6 : td == 16 ? 4 : 1;
    std::memcpy(m->tb.a, tables.data(), 36 * sizeof(double));
    std::memcpy(m->tb.b, tables.data() + 36, 36 * sizeof(double));
    std::memcpy(m->tb.c, tables.data() + 72, 36 * sizeof(double));
    std::memcpy(m->sc.s, tables.data() + 108, 16 * sizeof(double));

    const size_t total = (size_t)(2 * kMargin + (int64_t)td * n + 2);
    double* buf = static_cast<double*>(aligned_alloc(64, (total * sizeof(double) + 63) / 64 * 64));
    for (size_t i = 0; i < total; ++i) std::memcpy(buf + i, &kCanary, 8);
    double* tangent = buf + kMargin + off;
    for (int64_t i = 0; i < (int64_t)td * n; ++i) tangent[i] = std::numeric_limits<double>::quiet_NaN();

    ExpandPool* pool = host_tangent_pool(c);
    if (!pool || pool_threads(pool) != threads) return 3;
    const HostTangentJob job = host_tangent_job(m, tangent);
    if ((int)job.kind != kind || job.td != td) return 3;

    if (kind == HostTangentJob::CONST) {  // run_const_tangent
        pool_begin(pool, job);
        pool_post(pool, 0, n, nullptr, nullptr);
        pool_finish(pool);
    } else {
        const int prm = job.prm;
        const std::vector<double> params = read_file<double>(dir + "/params.f64");
        const std::vector<unsigned long long> ballots = read_file<unsigned long long>(dir + "/ballots.u64");
        const std::vector<int64_t> start = read_file<int64_t>(dir + "/starts.i64");
        const int64_t nchunks = (int64_t)start.size() - 1;
        if ((int64_t)params.size() != prm * n || (int64_t)ballots.size() != (n + 63) / 64 || nchunks < 1 || start.back() != n) return 2;
        int64_t chunk = 0;
        for (int64_t k = 0; k < nchunks; ++k) chunk = std::max(chunk, (start[(size_t)k + 1] - start[(size_t)k] + 63) / 64 * 64);
        if (host_tangent_ring(c, chunk, nslots, prm) != FCAMD_OK) return 3;
        const size_t slot_doubles = host_tangent_slot_doubles(chunk, prm);
        double* ring = reinterpret_cast<double*>(c->tparams);
        for (size_t i = 0; i < (size_t)nslots * slot_doubles; ++i) ring[i] = std::numeric_limits<double>::quiet_NaN();  // first use
        auto slot = [&](int64_t k) { return ring + (size_t)(k % nslots) * slot_doubles; };
        auto points = [&](int64_t k) { return start[(size_t)k + 1] - start[(size_t)k]; };
        // the kernel of chunk k: the parameters of the PLASTIC points of the launch's np points, every tile's ballot behind
        // prm * roundup(np, 64) doubles; every other double of the slot keeps what it held
        auto device = [&](int64_t k) {
            const int64_t p0 = start[(size_t)k], np = points(k);
            double* s = slot(k);
            unsigned long long* words = reinterpret_cast<unsigned long long*>(s + (size_t)prm * (size_t)((np + 63) / 64 * 64));
            for (int64_t l = 0; l < np; ++l)
                if ((ballots[(size_t)((p0 + l) >> 6)] >> ((p0 + l) & 63)) & 1ull)
                    std::memcpy(s + prm * l, params.data() + prm * (p0 + l), (size_t)prm * sizeof(double));
            for (int64_t w = 0; w < (np + 63) / 64; ++w) words[w] = ballots[(size_t)((p0 >> 6) + w)];
        };
        std::vector<int> ticket((size_t)nchunks, -1);
        auto post = [&](int64_t k) {
            const int64_t np = points(k);
            const unsigned long long* words = reinterpret_cast<const unsigned long long*>(slot(k) + (size_t)prm * (size_t)((np + 63) / 64 * 64));
            ticket[(size_t)k] = pool_post(pool, start[(size_t)k], np, slot(k), words);
        };
        pool_begin(pool, job);
        if (mode == 0) {
            for (int64_t k = 0; k < nchunks; ++k) {
                if (k >= nslots) pool_wait(pool, ticket[(size_t)(k - nslots)]);
                device(k);
                post(k);
            }
        } else {
            std::atomic<int64_t> launched{0}, done{0};  // chunks [0, launched) are enqueued, [0, done) have completed (the events)
            std::thread gpu([&] {
                for (int64_t k = 0; k < nchunks; ++k) {
                    while (launched.load(std::memory_order_acquire) <= k) std::this_thread::yield();
                    device(k);
                    done.store(k + 1, std::memory_order_release);
                }
            });
            int64_t posted = 0;
            auto query = [&](int64_t k) { return done.load(std::memory_order_acquire) > k; };  // hipEventQuery
            for (int64_t k = 0; k < nchunks; ++k) {
                while (posted < k && query(posted)) post(posted++);
                if (k >= nslots) {
                    while (posted <= k - nslots) {
                        while (!query(posted)) std::this_thread::yield();  // hipEventSynchronize
                        post(posted++);
                    }
                    pool_wait(pool, ticket[(size_t)(k - nslots)]);
                }
                launched.store(k + 1, std::memory_order_release);
            }
            while (posted < nchunks) {
                while (!query(posted)) std::this_thread::yield();
                post(posted++);
            }
            gpu.join();
        }
        pool_finish(pool);
    }
    printf("busy_us %lld threads %d\n", (long long)(pool_busy_seconds(pool) * 1e6), pool_threads(pool));

    FILE* f = fopen((dir + "/tangent.f64").c_str(), "wb");
    if (!f) return 2;
    const size_t count = (size_t)(2 * kMargin + (int64_t)td * n);
    const bool ok = fwrite(buf + off, sizeof(double), count, f) == count;
    fclose(f);
    host_tangent_release(c);
    free(buf);
    delete m;
    delete c;
    return ok ? 0 : 2;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "plan" && argc == 5) return cmd_plan(argv + 2);
    if (cmd == "plans" && argc == 2) return cmd_plans();
    if (cmd == "parts" && argc == 5) return cmd_parts(argv + 2);
    if (cmd == "run" && argc == 10) return cmd_run(argv + 2);
    fprintf(stderr, "usage: see the head of tests/host_tangent_harness.cpp\n");
    return 64;
}
