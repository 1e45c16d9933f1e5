// node.hip -- the receivers of one node: N channels split into contiguous blocks over the node's GPUs.
//
// gnuais creates its receivers one by one and they share nothing (src/ais.c:141-147); the main loop hands every
// receiver the same interleaved buffer (src/ais.c:237-247).  A node object is that for many devices: device g owns
// channels [first_g, first_g + n_g) as one gnuais_batch of its own, every device has ONE host thread that issues
// its copies and launches (hipSetDevice is per thread) on the batch's own streams, and nothing is exchanged
// between devices -- no collective, no peer copy.  What comes back is merged on the host: frame records with
// GLOBAL channel numbers in the reference's order (channel, then time), counters per global channel.
//
// Built on the public batch ABI only (include/gnuais_hip.h); the HIP runtime is used for the host-buffer split
// (a strided 2-D copy per device) and nothing else.
#ifndef _GNU_SOURCE
#define _GNU_SOURCE
#endif
#include <hip/hip_runtime.h>
#include <sched.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/gnuais_hip.h"

namespace {

thread_local std::string g_node_err;

int node_fail(int code, const std::string &what)
{
    g_node_err = what;
    return code;
}

double wall_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

struct Worker {
    std::thread th;
    std::mutex m;
    std::condition_variable cv;
    std::function<int()> job;
    bool has_job = false, done = true, quit = false;
    int rc = GNUAIS_OK;
    std::string err;

    void loop()
    {
        for (;;) {
            std::function<int()> j;
            {
                std::unique_lock<std::mutex> l(m);
                cv.wait(l, [&] { return has_job || quit; });
                if (quit) return;
                j = std::move(job);
                has_job = false;
            }
            g_node_err.clear();
            const int r = j();
            // the job's own message (node_fail: hipSetDevice, staging, copies) if it left one, else the batch layer's
            // (both are thread-local and this is the thread the job ran on)
            std::string e = r == GNUAIS_OK ? std::string() : (!g_node_err.empty() ? g_node_err : std::string(gnuais_last_error()));
            {
                std::lock_guard<std::mutex> l(m);
                rc = r;
                err = std::move(e);
                done = true;
            }
            cv.notify_all();
        }
    }
    void submit(std::function<int()> j)
    {
        {
            std::lock_guard<std::mutex> l(m);
            job = std::move(j);
            has_job = true;
            done = false;
        }
        cv.notify_all();
    }
    int wait()
    {
        std::unique_lock<std::mutex> l(m);
        cv.wait(l, [&] { return done; });
        return rc;
    }
};

struct Shard {
    int device = 0, first = 0, n = 0;
    gnuais_batch *b = nullptr;
    void *d_in = nullptr;                       // the host entries' slab (run_staged), in_bytes long
    size_t in_bytes = 0;
    hipStream_t s_in = nullptr;
    // where the shard's host thread runs: the NUMA node of its device (sysfs, via the device's PCI address) and how many
    // CPUs of that node the thread was pinned to (0: not pinned -- no sysfs entry, one node only, or GNUAIS_NODE_PIN=0)
    int numa_node = -1, pinned_cpus = 0;
    char pci[32] = {0};
    // since the last gnuais_node_mark(): calls, the host time spent inside the run calls (submission), and the wall clock
    // of the first submission and of the end of the shard's last sync -- so that one slow device shows by itself
    unsigned long long m_calls = 0;
    double m_submit_ms = 0.0, m_first = 0.0, m_last_sync = 0.0;
    Worker w;
};

// Books one submission into the shard's statistics: a call, and the host time until the booking goes out of scope
struct Booking {
    Shard &s;
    double t0 = wall_ms();
    explicit Booking(Shard &sh) : s(sh) { if (s.m_calls++ == 0) s.m_first = t0; }
    ~Booking() { s.m_submit_ms += wall_ms() - t0; }
};

// The input forms (include/gnuais_hip.h) as one shard sees them: a row of the caller's host array holds `cols` columns
// of `bytes` bytes each (a wide column: its sample format's pair), of which the shard owns [c0, c0 + nc); a chain row
// takes `rows` input rows
struct Form { int bytes, cols, c0, nc, rows; };
enum FormId { AUDIO, IQ, WIDE };

// "0-15,32-47" -> CPUs set in `set`; returns how many
int parse_cpulist(const char *text, cpu_set_t *set)
{
    int n = 0;
    CPU_ZERO(set);
    for (const char *p = text; *p;) {
        char *e;
        long a = strtol(p, &e, 10), b = a;
        if (e == p) break;
        if (*e == '-') b = strtol(e + 1, &e, 10);
        for (long c = a; c <= b && c < CPU_SETSIZE; ++c) { CPU_SET((int) c, set); ++n; }
        p = (*e == ',') ? e + 1 : e;
        if (*e != ',' ) break;
    }
    return n;
}

// Runs ON the shard's thread, before anything else: pin it to the CPUs of the NUMA node its device hangs off, so that
// what the thread allocates and touches from here on (the batch's pinned staging buffers, the launch path's queues)
// is local to that device's root complex.  Every step may fail quietly: the thread then stays where the OS put it.
void pin_to_device_node(Shard &s)
{
    if (hipDeviceGetPCIBusId(s.pci, (int) sizeof s.pci, s.device) != hipSuccess) { s.pci[0] = 0; return; }
    for (char *c = s.pci; *c; ++c) if (*c >= 'A' && *c <= 'F') *c = (char) (*c - 'A' + 'a');   // sysfs spells it lower case
    char path[160], buf[4096];
    snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", s.pci);
    FILE *f = fopen(path, "r");
    if (!f) return;
    int node = -1;
    if (fscanf(f, "%d", &node) != 1) node = -1;
    fclose(f);
    s.numa_node = node;
    const char *off = getenv("GNUAIS_NODE_PIN");
    if (node < 0 || (off && atoi(off) == 0)) return;
    snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
    f = fopen(path, "r");
    if (!f) return;
    const bool ok = fgets(buf, sizeof buf, f) != nullptr;
    fclose(f);
    if (!ok) return;
    cpu_set_t want, have, both;
    if (parse_cpulist(buf, &want) == 0 || sched_getaffinity(0, sizeof have, &have) != 0) return;
    CPU_AND(&both, &want, &have);               // only CPUs this process may use at all (cgroup / taskset)
    const int n = CPU_COUNT(&both);
    if (n > 0 && sched_setaffinity(0, sizeof both, &both) == 0) s.pinned_cpus = n;
}

} // namespace

struct gnuais_node {
    int N = 0, max_len = 0;
    int ch_K = 0, ch_D = 0, ch_U = 1;   // gnuais_node_channeliser / _resampler (ch_K == 0: not configured)
    std::vector<Shard *> shards;
    std::vector<gnuais_frame> scratch;
    std::string warnings;           // what create could not do without failing (one line per shard)
    // gnuais_node_unique: copies on different shards must merge and the shards exchange nothing, so the node merges on
    // the host -- the timed drain of every shard into these buffers, then one gnuais_uniq over the union
    gnuais_uniq *uq = nullptr;
    std::vector<gnuais_frame> uq_frames;
    std::vector<int64_t> uq_times;
    std::vector<gnuais_frame_signal> uq_signal;     // gnuais_node_drain_frames_heard: the members' records
    // gnuais_node_long_unique: the same for the long frames -- the shards' plain long drains, then one gnuais_long_uniq
    gnuais_long_uniq *lq = nullptr;
    std::vector<gnuais_long_frame> lq_frames;
    std::vector<gnuais_frame_signal> lq_signal;     // gnuais_node_drain_long_frames_heard: the members' records
};

extern "C" {

const char *gnuais_node_last_error(void) { return g_node_err.c_str(); }

static Form form(const gnuais_node *nd, const Shard &s, FormId f, int fmt = GNUAIS_FMT_CS16)
{
    const int K = f == WIDE ? nd->ch_K : 1;
    return {f == AUDIO ? 2 : f == IQ ? 4 : gnuais_sample_format_bytes(fmt), nd->N / K, s.first / K, s.n / K,
            f == WIDE ? nd->ch_D : 1};
}

// f(shard, its index) on every shard's own thread at once; the first failure is reported with the shard it came from
static int run_all(gnuais_node *nd, const std::function<int(Shard &, size_t)> &f)
{
    for (size_t i = 0; i < nd->shards.size(); ++i) {
        Shard *s = nd->shards[i];
        s->w.submit([s, i, &f] { return f(*s, i); });
    }
    int rc = GNUAIS_OK;
    for (Shard *s : nd->shards) {
        const int r = s->w.wait();
        if (r != GNUAIS_OK && rc == GNUAIS_OK) {
            rc = r;
            g_node_err = "device " + std::to_string(s->device) + " (channels " + std::to_string(s->first) + ".." +
                         std::to_string(s->first + s->n - 1) + "): " + s->w.err;
        }
    }
    return rc;
}

void gnuais_node_destroy(gnuais_node *nd)
{
    if (!nd) return;
    gnuais_uniq_destroy(nd->uq);
    gnuais_long_uniq_destroy(nd->lq);
    for (Shard *s : nd->shards) {
        if (s->w.th.joinable()) {
            s->w.submit([s] {
                (void) hipSetDevice(s->device);
                if (s->b) gnuais_batch_destroy(s->b);
                if (s->d_in) (void) hipFree(s->d_in);
                if (s->s_in) (void) hipStreamDestroy(s->s_in);
                return GNUAIS_OK;
            });
            s->w.wait();
            {
                std::lock_guard<std::mutex> l(s->w.m);
                s->w.quit = true;
            }
            s->w.cv.notify_all();
            s->w.th.join();
        }
        delete s;
    }
    delete nd;
}

int gnuais_node_create(gnuais_node **out, const int *devices, int n_devices, int n_channels, const float *taps,
                       int n_taps, unsigned pllinc, int max_len, int frame_capacity_per_device)
{
    if (!out) return node_fail(GNUAIS_E_ARG, "node_create: out is NULL");
    *out = nullptr;
    if (n_channels <= 0 || max_len <= 0) return node_fail(GNUAIS_E_ARG, "node_create: n_channels / max_len");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return node_fail(GNUAIS_E_HIP, "node_create: no HIP device");
    std::vector<int> devs;
    if (devices && n_devices > 0) devs.assign(devices, devices + n_devices);
    else for (int d = 0; d < ndev; ++d) devs.push_back(d);            // NULL / 0: every visible device
    for (int d : devs)
        if (d < 0 || d >= ndev) return node_fail(GNUAIS_E_ARG, "node_create: device index out of range");
    const int G = (int) std::min<size_t>(devs.size(), (size_t) n_channels);
    gnuais_node *nd = new gnuais_node;
    nd->N = n_channels;
    nd->max_len = max_len;
    for (int g = 0; g < G; ++g) {
        // contiguous blocks, SURVEY 8e: device g owns [g*N/G, (g+1)*N/G)
        const int lo = (int) ((long long) n_channels * g / G), hi = (int) ((long long) n_channels * (g + 1) / G);
        Shard *s = new Shard;
        s->device = devs[g];
        s->first = lo;
        s->n = hi - lo;
        s->w.th = std::thread([s] { pin_to_device_node(*s); s->w.loop(); });
        nd->shards.push_back(s);
    }
    const int rc = run_all(nd, [&](Shard &s, size_t) {
        return gnuais_batch_create(&s.b, s.device, s.n, taps, n_taps, pllinc, max_len, frame_capacity_per_device);
    });
    if (rc != GNUAIS_OK) {
        const std::string keep = g_node_err;
        gnuais_node_destroy(nd);
        return node_fail(rc, keep);
    }
    // not fatal, but worth knowing before a scaling curve is read: a shard whose host thread stayed where the OS put it
    // (no NUMA node in sysfs, no CPU of that node in this process's affinity mask, GNUAIS_NODE_PIN=0)
    for (size_t g = 0; g < nd->shards.size(); ++g) {
        const Shard *s = nd->shards[g];
        if (s->pinned_cpus == 0 && nd->shards.size() > 1) {
            char line[200];
            snprintf(line, sizeof line, "shard %zu (device %d, pci %s): host thread not pinned (numa_node %d)\n", g, s->device,
                     s->pci[0] ? s->pci : "?", s->numa_node);
            nd->warnings += line;
        }
    }
    *out = nd;
    return GNUAIS_OK;
}

const char *gnuais_node_warnings(const gnuais_node *nd) { return nd ? nd->warnings.c_str() : ""; }

int gnuais_node_n_devices(const gnuais_node *nd) { return nd ? (int) nd->shards.size() : 0; }
int gnuais_node_n_channels(const gnuais_node *nd) { return nd ? nd->N : 0; }

int gnuais_node_shard(const gnuais_node *nd, int i, int *device, int *first_channel, int *n_channels,
                      gnuais_batch **batch)
{
    if (!nd || i < 0 || i >= (int) nd->shards.size()) return node_fail(GNUAIS_E_ARG, "node_shard: index");
    const Shard *s = nd->shards[i];
    if (device) *device = s->device;
    if (first_channel) *first_channel = s->first;
    if (n_channels) *n_channels = s->n;
    if (batch) *batch = s->b;
    return GNUAIS_OK;
}

int gnuais_node_reset(gnuais_node *nd)
{
    if (!nd) return node_fail(GNUAIS_E_ARG, "node_reset: NULL");
    if (nd->uq) (void) gnuais_uniq_reset(nd->uq);
    if (nd->lq) (void) gnuais_long_uniq_reset(nd->lq);
    return run_all(nd, [](Shard &s, size_t) { return gnuais_batch_reset(s.b); });
}

// gnuais_node_run / _run_iq: shard i runs `run`, the batch entry of the form, on its device slab slabs[i] and streams[i]
static int run_slabs(gnuais_node *nd, const int16_t *const *slabs, int len, void *const *streams, const char *who,
                     int (*run)(gnuais_batch *, const int16_t *, int, void *))
{
    if (!nd || !slabs) return node_fail(GNUAIS_E_ARG, std::string(who) + ": NULL argument");
    if (len <= 0 || len > nd->max_len) return node_fail(GNUAIS_E_ARG, std::string(who) + ": len out of range");
    return run_all(nd, [&](Shard &s, size_t i) {
        Booking book(s);
        return run(s.b, slabs[i], len, streams ? streams[i] : nullptr);
    });
}

// The host entries: on the shard's input stream s_in, the shard's columns of the caller's host array go into the
// shard's slab by one strided 2-D copy, then `run`, the batch entry of the form, reads them there.  Everything that
// reads the slab runs on s_in (K1, the discriminator, the channeliser), and every call syncs s_in before it returns,
// so the slab is free again between calls: one slab serves every form, sized for max_len chain rows of the widest one.
// run == NULL: the wide form in sample format fmt, through gnuais_batch_run_wideband_fmt
static int run_staged(gnuais_node *nd, FormId id, const void *h, int len, const char *who,
                      int (*run)(gnuais_batch *, const int16_t *, int, void *), int fmt = GNUAIS_FMT_CS16)
{
    return run_all(nd, [=](Shard &s, size_t) -> int {
        Booking book(s);
        auto hip_fail = [&](const char *what) { return node_fail(GNUAIS_E_HIP, std::string(who) + ": " + what); };
        const Form f = form(nd, s, id, fmt);
        if (hipSetDevice(s.device) != hipSuccess) return hip_fail("hipSetDevice");
        if (!s.s_in && hipStreamCreateWithFlags(&s.s_in, hipStreamNonBlocking) != hipSuccess) return hip_fail("stream");
        const size_t row = (size_t) f.bytes * (size_t) f.nc, need = row * (size_t) f.rows * (size_t) nd->max_len;
        if (s.in_bytes < need) {
            if (s.d_in) (void) hipFree(s.d_in);
            s.d_in = nullptr;
            s.in_bytes = 0;
            if (hipMalloc(&s.d_in, need) != hipSuccess) return hip_fail("staging allocation");
            s.in_bytes = need;
        }
        const char *src = (const char *) h + (size_t) f.bytes * (size_t) f.c0;
        if (hipMemcpy2DAsync(s.d_in, row, src, (size_t) f.bytes * (size_t) f.cols, row, (size_t) len, hipMemcpyHostToDevice,
                             s.s_in) != hipSuccess)
            return hip_fail("host -> device copy");
        const int rc = run ? run(s.b, (const int16_t *) s.d_in, len, s.s_in)
                           : gnuais_batch_run_wideband_fmt(s.b, fmt, s.d_in, len, s.s_in);
        // the caller's buffer is borrowed for the call only (src/ais.c:216 reuses it): the copy out of it must be done
        if (hipStreamSynchronize(s.s_in) != hipSuccess && rc == GNUAIS_OK) return hip_fail("copy");
        return rc;
    });
}

int gnuais_node_run(gnuais_node *nd, const int16_t *const *d_samples, int len, void *const *streams)
{
    return run_slabs(nd, d_samples, len, streams, "node_run", gnuais_batch_run);
}

int gnuais_node_run_iq(gnuais_node *nd, const int16_t *const *d_iq, int len, void *const *streams)
{
    return run_slabs(nd, d_iq, len, streams, "node_run_iq", gnuais_batch_run_iq);
}

int gnuais_node_run_host(gnuais_node *nd, const int16_t *h_samples, int len)
{
    if (!nd || !h_samples) return node_fail(GNUAIS_E_ARG, "node_run_host: NULL argument");
    if (len <= 0 || len > nd->max_len) return node_fail(GNUAIS_E_ARG, "node_run_host: len out of range");
    return run_staged(nd, AUDIO, h_samples, len, "node_run_host", gnuais_batch_run);
}

int gnuais_node_run_iq_host(gnuais_node *nd, const int16_t *h_iq, int len)
{
    if (!nd || !h_iq) return node_fail(GNUAIS_E_ARG, "node_run_iq_host: NULL argument");
    if (len <= 0 || len > nd->max_len) return node_fail(GNUAIS_E_ARG, "node_run_iq_host: len out of range");
    return run_staged(nd, IQ, h_iq, len, "node_run_iq_host", gnuais_batch_run_iq);
}

// gnuais_node_channeliser / _resampler: the shards' rule, then `configure` on every shard's batch; `who`: the entry's name
static int node_wide_configure(gnuais_node *nd, const char *who, int up, int down, const int32_t *offsets_hz, int n_offsets,
                               const std::function<int(gnuais_batch *)> &configure)
{
    if (!nd || !offsets_hz) return node_fail(GNUAIS_E_ARG, std::string(who) + ": NULL argument");
    if (n_offsets < 1) return node_fail(GNUAIS_E_ARG, std::string(who) + ": n_offsets must be >= 1");
    for (size_t i = 0; i < nd->shards.size(); ++i) {
        const Shard &s = *nd->shards[i];
        if (s.first % n_offsets || s.n % n_offsets) {
            char msg[200];
            snprintf(msg, sizeof msg, "%s: shard %zu (channels %d..%d) does not start and end on a multiple of "
                     "n_offsets = %d", who, i, s.first, s.first + s.n - 1, n_offsets);
            return node_fail(GNUAIS_E_ARG, msg);
        }
    }
    nd->ch_K = 0;
    const int rc = run_all(nd, [&](Shard &s, size_t) { return configure(s.b); });
    if (rc == GNUAIS_OK) {
        nd->ch_K = n_offsets;
        nd->ch_D = down;
        nd->ch_U = up;
    }
    return rc;
}

int gnuais_node_channeliser(gnuais_node *nd, int decim, int in_rate_hz, const int32_t *offsets_hz, int n_offsets,
                            const int16_t *taps, int n_taps)
{
    return node_wide_configure(nd, "node_channeliser", 1, decim, offsets_hz, n_offsets, [=](gnuais_batch *b) {
        return gnuais_batch_channeliser(b, decim, in_rate_hz, offsets_hz, n_offsets, taps, n_taps);
    });
}

int gnuais_node_resampler(gnuais_node *nd, int up, int down, int in_rate_hz, const int32_t *offsets_hz, int n_offsets,
                          const int16_t *taps, int n_taps)
{
    return node_wide_configure(nd, "node_resampler", up, down, offsets_hz, n_offsets, [=](gnuais_batch *b) {
        return gnuais_batch_resampler(b, up, down, in_rate_hz, offsets_hz, n_offsets, taps, n_taps);
    });
}

int gnuais_node_afc(gnuais_node *nd, int window)
{
    if (!nd) return node_fail(GNUAIS_E_ARG, "node_afc: NULL node");
    return run_all(nd, [=](Shard &s, size_t) { return gnuais_batch_afc(s.b, window); });
}

// a wideband call's length against the node's configuration (gnuais_node_channeliser: U = 1; gnuais_node_resampler)
static int wide_len_check(const gnuais_node *nd, int len, const char *who)
{
    if (len > 0 && len % nd->ch_D == 0 && (long long) (len / nd->ch_D) * nd->ch_U <= nd->max_len) return GNUAIS_OK;
    char msg[240];
    if (nd->ch_U == 1)
        snprintf(msg, sizeof msg, "%s: len must be a positive multiple of the decimation, at most decim * max_len", who);
    else
        snprintf(msg, sizeof msg, "%s: len %d must be a positive multiple of down = %d that gives at most max_len rows "
                 "(len * %d / %d <= %d)", who, len, nd->ch_D, nd->ch_U, nd->ch_D, nd->max_len);
    return node_fail(GNUAIS_E_ARG, msg);
}

int gnuais_node_run_wideband_host(gnuais_node *nd, const int16_t *h_wide, int len)
{
    if (!nd || !h_wide) return node_fail(GNUAIS_E_ARG, "node_run_wideband_host: NULL argument");
    if (!nd->ch_K) return node_fail(GNUAIS_E_ARG, "node_run_wideband_host: no channeliser configured (gnuais_node_channeliser / _resampler)");
    if (int rc = wide_len_check(nd, len, "node_run_wideband_host")) return rc;
    return run_staged(nd, WIDE, h_wide, len, "node_run_wideband_host", gnuais_batch_run_wideband);
}

int gnuais_node_run_wideband_fmt_host(gnuais_node *nd, int fmt, const void *h_wide, int len)
{
    if (!nd || !h_wide) return node_fail(GNUAIS_E_ARG, "node_run_wideband_fmt_host: NULL argument");
    if (gnuais_sample_format_bytes(fmt) < 0)
        return node_fail(GNUAIS_E_ARG, "node_run_wideband_fmt_host: unknown sample format (GNUAIS_FMT_*)");
    if (!nd->ch_K) return node_fail(GNUAIS_E_ARG, "node_run_wideband_fmt_host: no channeliser configured (gnuais_node_channeliser / _resampler)");
    if (int rc = wide_len_check(nd, len, "node_run_wideband_fmt_host")) return rc;
    return run_staged(nd, WIDE, h_wide, len, "node_run_wideband_fmt_host", nullptr, fmt);
}

int gnuais_node_sync(gnuais_node *nd)
{
    if (!nd) return node_fail(GNUAIS_E_ARG, "node_sync: NULL");
    return run_all(nd, [](Shard &s, size_t) {
        const int rc = gnuais_batch_sync(s.b);
        s.m_last_sync = wall_ms();
        return rc;
    });
}

// Per-shard bookkeeping for whoever times a node (bench.py --gpus N): gnuais_node_mark() starts a measurement,
// gnuais_node_shard_stats() reads one shard's after a gnuais_node_sync().
int gnuais_node_mark(gnuais_node *nd)
{
    if (!nd) return node_fail(GNUAIS_E_ARG, "node_mark: NULL");
    return run_all(nd, [](Shard &s, size_t) {
        s.m_calls = 0;
        s.m_submit_ms = s.m_first = s.m_last_sync = 0.0;
        return GNUAIS_OK;
    });
}

int gnuais_node_shard_stats(const gnuais_node *nd, int i, gnuais_node_shard_stat *out)
{
    if (!nd || !out || i < 0 || i >= (int) nd->shards.size()) return node_fail(GNUAIS_E_ARG, "node_shard_stats: argument");
    const Shard *s = nd->shards[i];
    memset(out, 0, sizeof *out);
    out->device = s->device;
    out->first_channel = s->first;
    out->n_channels = s->n;
    out->numa_node = s->numa_node;
    out->pinned_cpus = s->pinned_cpus;
    out->calls = (long long) s->m_calls;
    out->submit_ms = s->m_submit_ms;
    out->busy_ms = (s->m_calls && s->m_last_sync > s->m_first) ? s->m_last_sync - s->m_first : 0.0;
    snprintf(out->pci, sizeof out->pci, "%s", s->pci);
    return GNUAIS_OK;
}

int gnuais_node_pending_frames(gnuais_node *nd, int *n_out)
{
    if (!nd || !n_out) return node_fail(GNUAIS_E_ARG, "node_pending_frames: argument");
    std::vector<int> n(nd->shards.size(), 0);
    const int rc = run_all(nd, [&](Shard &s, size_t i) { return gnuais_batch_pending_frames(s.b, &n[i]); });
    long long t = 0;
    for (int v : n) t += v;
    *n_out = (int) std::min<long long>(t, 0x7fffffff);
    return rc;
}

int gnuais_node_frame_times(gnuais_node *nd, int on)
{
    if (!nd) return node_fail(GNUAIS_E_ARG, "node_frame_times: NULL node");
    if (!on && nd->uq) return node_fail(GNUAIS_E_STATE, "node_frame_times: the node merges duplicates by their times (gnuais_node_unique)");
    return run_all(nd, [=](Shard &s, size_t) { return gnuais_batch_frame_times(s.b, on); });
}

int gnuais_node_frame_signal(gnuais_node *nd, int on)
{
    if (!nd) return node_fail(GNUAIS_E_ARG, "node_frame_signal: NULL node");
    return run_all(nd, [=](Shard &s, size_t) { return gnuais_batch_frame_signal(s.b, on); });
}

int gnuais_node_occupancy(gnuais_node *nd, int epoch_blocks, int margin)
{
    if (!nd) return node_fail(GNUAIS_E_ARG, "node_occupancy: NULL node");
    return run_all(nd, [=](Shard &s, size_t) { return gnuais_batch_occupancy(s.b, epoch_blocks, margin); });
}

// every shard's final epochs into a buffer of its own, then laid side by side by global channel: the shards took the same
// rows, so they made the same epochs final
int gnuais_node_drain_occupancy(gnuais_node *nd, gnuais_occupancy *h_out, int64_t *h_first_block, int max, int *n_out)
{
    if (!nd || !n_out || max < 0 || (max > 0 && (!h_out || !h_first_block)))
        return node_fail(GNUAIS_E_ARG, "node_drain_occupancy: argument");
    *n_out = 0;
    std::vector<Shard *> &sh = nd->shards;
    std::vector<std::vector<gnuais_occupancy>> rec(sh.size());
    std::vector<std::vector<int64_t>> first(sh.size());
    std::vector<int> cnt(sh.size(), 0);
    const int rc = run_all(nd, [&](Shard &s, size_t i) {
        rec[i].resize((size_t) std::max(max, 1) * (size_t) s.n);
        first[i].resize((size_t) std::max(max, 1));
        return gnuais_batch_drain_occupancy(s.b, rec[i].data(), first[i].data(), max, &cnt[i]);
    });
    if (rc) return rc;
    for (size_t i = 1; i < sh.size(); ++i)
        if (cnt[i] != cnt[0] || !std::equal(first[i].begin(), first[i].begin() + cnt[i], first[0].begin()))
            return node_fail(GNUAIS_E_STATE, "node_drain_occupancy: the shards' epochs do not align");
    for (int k = 0; k < cnt[0]; ++k) {
        h_first_block[k] = first[0][(size_t) k];
        for (size_t i = 0; i < sh.size(); ++i)
            memcpy(h_out + (size_t) k * (size_t) nd->N + (size_t) sh[i]->first, rec[i].data() + (size_t) k * (size_t) sh[i]->n,
                   sizeof(gnuais_occupancy) * (size_t) sh[i]->n);
    }
    *n_out = cnt[0];
    return GNUAIS_OK;
}

int gnuais_node_repair(gnuais_node *nd, int on)
{
    if (!nd) return node_fail(GNUAIS_E_ARG, "node_repair: NULL node");
    return run_all(nd, [=](Shard &s, size_t) { return gnuais_batch_repair(s.b, on); });
}

int gnuais_node_repaired(gnuais_node *nd, int32_t *h_out)
{
    if (!nd || !h_out) return node_fail(GNUAIS_E_ARG, "node_repaired: argument");
    return run_all(nd, [&](Shard &s, size_t) { return gnuais_batch_repaired(s.b, h_out + s.first); });
}

// messages of three to five slots (gnuais_batch_long_frames on every shard)
int gnuais_node_long_frames(gnuais_node *nd, int on)
{
    if (!nd) return node_fail(GNUAIS_E_ARG, "node_long_frames: NULL node");
    // any switch empties gnuais_node_long_unique's carried state; switching long frames off switches that off
    if (nd->lq) (void) gnuais_long_uniq_reset(nd->lq);
    if (!on) {
        gnuais_long_uniq_destroy(nd->lq);
        nd->lq = nullptr;
    }
    return run_all(nd, [=](Shard &s, size_t) { return gnuais_batch_long_frames(s.b, on); });
}

int gnuais_node_long_counters(gnuais_node *nd, int32_t *h_delivered, int32_t *h_failed)
{
    if (!nd || !h_delivered || !h_failed) return node_fail(GNUAIS_E_ARG, "node_long_counters: argument");
    return run_all(nd, [&](Shard &s, size_t) { return gnuais_batch_long_counters(s.b, h_delivered + s.first, h_failed + s.first); });
}

// the repair of long frames (gnuais_batch_long_repair on every shard) and the repairs per global channel
int gnuais_node_long_repair(gnuais_node *nd, int on)
{
    if (!nd) return node_fail(GNUAIS_E_ARG, "node_long_repair: NULL node");
    return run_all(nd, [=](Shard &s, size_t) { return gnuais_batch_long_repair(s.b, on); });
}

int gnuais_node_long_repaired(gnuais_node *nd, int32_t *h_out)
{
    if (!nd || !h_out) return node_fail(GNUAIS_E_ARG, "node_long_repaired: argument");
    return run_all(nd, [&](Shard &s, size_t) { return gnuais_batch_long_repaired(s.b, h_out + s.first); });
}

// every shard drains its own long ring; a shard's records come in (channel, stamp) order with LOCAL channel numbers and
// the shards own ascending channel blocks, so the parts are renumbered and laid end to end
static int node_drain_long(gnuais_node *nd, gnuais_long_frame *h_out, gnuais_frame_signal *h_signal, int max, int *n_out)
{
    *n_out = 0;
    std::vector<Shard *> &sh = nd->shards;
    std::vector<int> pend(sh.size(), 0);
    if (int rc = run_all(nd, [&](Shard &s, size_t i) { return gnuais_batch_pending_long_frames(s.b, &pend[i]); })) return rc;
    long long total = 0;
    for (int v : pend) total += v;
    if (total > max) return node_fail(GNUAIS_E_ARG, "node_drain_long_frames: frame buffer too small");
    std::vector<std::vector<gnuais_long_frame>> part(sh.size());
    std::vector<std::vector<gnuais_frame_signal>> part_s(sh.size());
    std::vector<int> cnt(sh.size(), 0);
    const int rc = run_all(nd, [&](Shard &s, size_t i) {
        part[i].resize((size_t) std::max(pend[i], 1));
        if (h_signal) part_s[i].resize((size_t) std::max(pend[i], 1));
        const int r = h_signal ? gnuais_batch_drain_long_frames_signal(s.b, part[i].data(), part_s[i].data(), pend[i], &cnt[i])
                               : gnuais_batch_drain_long_frames(s.b, part[i].data(), pend[i], &cnt[i]);
        for (int k = 0; k < cnt[i]; ++k) part[i][(size_t) k].channel += (uint32_t) s.first;
        return r;
    });
    int w = 0;
    for (size_t i = 0; i < sh.size(); ++i) {
        if (cnt[i] > 0) memcpy(h_out + w, part[i].data(), sizeof(gnuais_long_frame) * (size_t) cnt[i]);
        if (cnt[i] > 0 && h_signal) memcpy(h_signal + w, part_s[i].data(), sizeof(gnuais_frame_signal) * (size_t) cnt[i]);
        w += cnt[i];
    }
    *n_out = w;
    return rc;              // GNUAIS_E_OVERFLOW of a device is reported with what was drained
}

int gnuais_node_drain_long_frames(gnuais_node *nd, gnuais_long_frame *h_out, int max, int *n_out)
{
    if (!nd || !n_out || max < 0 || (max && !h_out)) return node_fail(GNUAIS_E_ARG, "node_drain_long_frames: argument");
    return node_drain_long(nd, h_out, nullptr, max, n_out);
}

// gnuais_batch_long_frame_signal on every shard, and the long drain with every record's power and carrier error
int gnuais_node_long_frame_signal(gnuais_node *nd, int on)
{
    if (!nd) return node_fail(GNUAIS_E_ARG, "node_long_frame_signal: NULL node");
    return run_all(nd, [=](Shard &s, size_t) { return gnuais_batch_long_frame_signal(s.b, on); });
}

int gnuais_node_drain_long_frames_signal(gnuais_node *nd, gnuais_long_frame *h_out, gnuais_frame_signal *h_signal, int max,
                                         int *n_out)
{
    if (!nd || !n_out || max < 0 || (max && (!h_out || !h_signal)))
        return node_fail(GNUAIS_E_ARG, "node_drain_long_frames_signal: argument");
    return node_drain_long(nd, h_out, h_signal, max, n_out);
}

static int node_drain(gnuais_node *nd, gnuais_frame *h_out, int64_t *h_times, int max, int *n_out,
                      gnuais_frame_signal *h_signal = nullptr);

int gnuais_node_drain_frames(gnuais_node *nd, gnuais_frame *h_out, int max, int *n_out)
{
    if (!nd || !h_out || !n_out || max < 0) return node_fail(GNUAIS_E_ARG, "node_drain_frames: argument");
    return node_drain(nd, h_out, nullptr, max, n_out);
}

// the same with every record's receive time (gnuais_batch_drain_frames_timed on every shard): every shard counts the
// rows of its own calls, and a node's run calls give every shard the same rows
int gnuais_node_drain_frames_timed(gnuais_node *nd, gnuais_frame *h_out, int64_t *h_times, int max, int *n_out)
{
    if (!nd || !h_out || !h_times || !n_out || max < 0) return node_fail(GNUAIS_E_ARG, "node_drain_frames_timed: argument");
    return node_drain(nd, h_out, h_times, max, n_out);
}

// and with every record's power and carrier error (gnuais_batch_drain_frames_signal on every shard)
int gnuais_node_drain_frames_signal(gnuais_node *nd, gnuais_frame *h_out, int64_t *h_times, gnuais_frame_signal *h_signal,
                                    int max, int *n_out)
{
    if (!nd || !h_out || !h_times || !h_signal || !n_out || max < 0)
        return node_fail(GNUAIS_E_ARG, "node_drain_frames_signal: argument");
    return node_drain(nd, h_out, h_times, max, n_out, h_signal);
}

static int node_drain(gnuais_node *nd, gnuais_frame *h_out, int64_t *h_times, int max, int *n_out, gnuais_frame_signal *h_signal)
{
    *n_out = 0;
    int total = 0;
    if (int rc = gnuais_node_pending_frames(nd, &total)) return rc;
    if (total > max) return node_fail(GNUAIS_E_ARG, "node_drain_frames: frame buffer too small");
    // every device drains into its own part of the output, concurrently; a shard's records come in the reference's
    // order (channel, then time) with LOCAL channel numbers, so the parts only have to be laid end to end -- shards
    // own ascending channel blocks -- and renumbered
    std::vector<Shard *> &sh = nd->shards;
    std::vector<int> cnt(sh.size(), 0), off(sh.size(), 0);
    {
        std::vector<int> pend(sh.size(), 0);
        const int rc = run_all(nd, [&](Shard &s, size_t i) { return gnuais_batch_pending_frames(s.b, &pend[i]); });
        if (rc) return rc;
        int o = 0;
        for (size_t i = 0; i < sh.size(); ++i) { off[i] = o; o += pend[i]; }
        if (o > max) return node_fail(GNUAIS_E_ARG, "node_drain_frames: frame buffer too small");
        cnt = pend;
    }
    const int rc = run_all(nd, [&](Shard &s, size_t i) {
        int got = 0;
        const int r = h_signal ? gnuais_batch_drain_frames_signal(s.b, h_out + off[i], h_times + off[i], h_signal + off[i], cnt[i], &got)
                      : h_times ? gnuais_batch_drain_frames_timed(s.b, h_out + off[i], h_times + off[i], cnt[i], &got)
                                : gnuais_batch_drain_frames(s.b, h_out + off[i], cnt[i], &got);
        for (int k = 0; k < got; ++k) h_out[off[i] + k].channel += (uint32_t) s.first;
        cnt[i] = got;
        return r;
    });
    // close gaps if a device delivered fewer than it had announced (it cannot deliver more)
    int w = 0;
    for (size_t i = 0; i < sh.size(); ++i) {
        if (off[i] != w && cnt[i] > 0) memmove(h_out + w, h_out + off[i], sizeof(gnuais_frame) * (size_t) cnt[i]);
        if (off[i] != w && cnt[i] > 0 && h_times) memmove(h_times + w, h_times + off[i], sizeof(int64_t) * (size_t) cnt[i]);
        if (off[i] != w && cnt[i] > 0 && h_signal) memmove(h_signal + w, h_signal + off[i], sizeof(gnuais_frame_signal) * (size_t) cnt[i]);
        w += cnt[i];
    }
    *n_out = w;
    return rc;              // GNUAIS_E_OVERFLOW of a device is reported with what was drained
}

// One record per transmission over the whole node (gnuais_batch_unique's definition): the merged timed drain, then the
// host object.  window_rows = 0 switches it off; switching clears the tail and the late count.
int gnuais_node_unique(gnuais_node *nd, int window_rows)
{
    if (!nd || window_rows < 0) return node_fail(GNUAIS_E_ARG, "node_unique: NULL node or a negative window");
    if (window_rows)
        for (Shard *s : nd->shards) {
            double on = 0;
            if (gnuais_batch_info(s->b, "frame_times", &on) != GNUAIS_OK || on == 0)
                return node_fail(GNUAIS_E_STATE, "node_unique: the node does not time its frames (gnuais_node_frame_times)");
        }
    gnuais_uniq_destroy(nd->uq);
    nd->uq = nullptr;
    if (window_rows && gnuais_uniq_create(&nd->uq, window_rows) != GNUAIS_OK)
        return node_fail(GNUAIS_E_ARG, "node_unique: the merge object could not be made");
    return GNUAIS_OK;
}

int gnuais_node_unique_late(gnuais_node *nd, long long *late)
{
    if (!nd || !late) return node_fail(GNUAIS_E_ARG, "node_unique_late: argument");
    *late = gnuais_uniq_late(nd->uq);
    return GNUAIS_OK;
}

// h_first: with the clusters' member lists (gnuais_node_drain_frames_heard)
static int node_drain_unique(gnuais_node *nd, gnuais_frame *h_out, int64_t *h_times, int32_t *h_copies, int max, int *n_out,
                             int32_t *h_first, gnuais_hearer *h_members, int *n_members)
{
    *n_out = 0;
    if (!nd->uq) return node_fail(GNUAIS_E_STATE, "node_drain_frames_unique: the node does not merge duplicates (gnuais_node_unique)");
    int total = 0;
    if (int rc = gnuais_node_pending_frames(nd, &total)) return rc;
    if (total > max) return node_fail(GNUAIS_E_ARG, "node_drain_frames_unique: buffers too small (one entry per pending frame always suffices)");
    nd->uq_frames.resize((size_t) total + 1);
    nd->uq_times.resize((size_t) total + 1);
    int got = 0;
    // the lists carry every copy's signal record: the shards' signal drain where they measure their frames, else zeros
    bool measured = h_first != nullptr;
    for (Shard *s : nd->shards) {
        double on = 0;
        if (measured && (gnuais_batch_info(s->b, "frame_signal", &on) != GNUAIS_OK || on == 0)) measured = false;
    }
    if (measured) nd->uq_signal.resize((size_t) total + 1);
    const int rc = node_drain(nd, nd->uq_frames.data(), nd->uq_times.data(), total, &got, measured ? nd->uq_signal.data() : nullptr);
    if (rc != GNUAIS_OK && rc != GNUAIS_E_OVERFLOW) return rc;
    double rows = 0;                    // a node's run calls give every shard the same rows
    if (gnuais_batch_info(nd->shards[0]->b, "rows", &rows) != GNUAIS_OK) return node_fail(GNUAIS_E_STATE, "node_drain_frames_unique: rows");
    const int pushed = h_first ? gnuais_uniq_push_heard(nd->uq, nd->uq_frames.data(), nd->uq_times.data(),
                                                        measured ? nd->uq_signal.data() : nullptr, got, (long long) rows, h_out,
                                                        h_times, h_copies, max, n_out, h_first, h_members, n_members)
                               : gnuais_uniq_push(nd->uq, nd->uq_frames.data(), nd->uq_times.data(), got, (long long) rows, h_out,
                                                  h_times, h_copies, max, n_out);
    if (pushed != GNUAIS_OK) return node_fail(GNUAIS_E_ARG, "node_drain_frames_unique: the merge refused its input");
    return rc;              // GNUAIS_E_OVERFLOW of a device is reported with what was drained
}

int gnuais_node_drain_frames_unique(gnuais_node *nd, gnuais_frame *h_out, int64_t *h_times, int32_t *h_copies, int max,
                                    int *n_out)
{
    if (!nd || !n_out || max < 0 || (max > 0 && (!h_out || !h_times || !h_copies)))
        return node_fail(GNUAIS_E_ARG, "node_drain_frames_unique: argument");
    return node_drain_unique(nd, h_out, h_times, h_copies, max, n_out, nullptr, nullptr, nullptr);
}

int gnuais_node_drain_frames_heard(gnuais_node *nd, gnuais_frame *h_out, int64_t *h_times, int32_t *h_copies, int max,
                                   int *n_out, int32_t *h_first, gnuais_hearer *h_members, int *n_members)
{
    if (!nd || !n_out || !n_members || !h_first || max < 0 || (max > 0 && (!h_out || !h_times || !h_copies || !h_members)))
        return node_fail(GNUAIS_E_ARG, "node_drain_frames_heard: argument");
    *n_members = 0;
    h_first[0] = 0;
    return node_drain_unique(nd, h_out, h_times, h_copies, max, n_out, h_first, h_members, n_members);
}

// One record per long transmission over the whole node (gnuais_batch_long_unique's definition): the shards' plain long
// drains merged, then the host object.  window_rows = 0 switches it off; switching clears the tail and the late count.
int gnuais_node_long_unique(gnuais_node *nd, int window_rows)
{
    if (!nd || window_rows < 0) return node_fail(GNUAIS_E_ARG, "node_long_unique: NULL node or a negative window");
    for (Shard *s : nd->shards) {
        double on = 0;
        if (gnuais_batch_info(s->b, "long_frames", &on) != GNUAIS_OK || on == 0)
            return node_fail(GNUAIS_E_STATE, "node_long_unique: the node does not decode long frames (gnuais_node_long_frames)");
    }
    gnuais_long_uniq_destroy(nd->lq);
    nd->lq = nullptr;
    if (window_rows && gnuais_long_uniq_create(&nd->lq, window_rows) != GNUAIS_OK)
        return node_fail(GNUAIS_E_ARG, "node_long_unique: the merge object could not be made");
    return GNUAIS_OK;
}

int gnuais_node_long_unique_late(gnuais_node *nd, long long *late)
{
    if (!nd || !late) return node_fail(GNUAIS_E_ARG, "node_long_unique_late: argument");
    *late = gnuais_long_uniq_late(nd->lq);
    return GNUAIS_OK;
}

// h_first: with the clusters' member lists (gnuais_node_drain_long_frames_heard)
static int node_drain_long_unique(gnuais_node *nd, gnuais_long_frame *h_out, int32_t *h_copies, int max, int *n_out,
                                  int32_t *h_first, gnuais_hearer *h_members, int *n_members)
{
    *n_out = 0;
    if (!nd->lq) return node_fail(GNUAIS_E_STATE, "node_drain_long_frames_unique: the node does not merge long frames (gnuais_node_long_unique)");
    std::vector<int> pend(nd->shards.size(), 0);
    if (int rc = run_all(nd, [&](Shard &s, size_t i) { return gnuais_batch_pending_long_frames(s.b, &pend[i]); })) return rc;
    long long total = 0;
    for (int v : pend) total += v;
    if (total > max) return node_fail(GNUAIS_E_ARG, "node_drain_long_frames_unique: buffers too small (one entry per pending long frame always suffices)");
    nd->lq_frames.resize((size_t) total + 1);
    int got = 0;
    // the lists carry every copy's signal record: the shards' signal drain where they measure their long frames, else zeros
    bool measured = h_first != nullptr;
    for (Shard *s : nd->shards) {
        double on = 0;
        if (measured && (gnuais_batch_info(s->b, "long_frame_signal", &on) != GNUAIS_OK || on == 0)) measured = false;
    }
    if (measured) nd->lq_signal.resize((size_t) total + 1);
    const int rc = node_drain_long(nd, nd->lq_frames.data(), measured ? nd->lq_signal.data() : nullptr, (int) total, &got);
    if (rc != GNUAIS_OK && rc != GNUAIS_E_OVERFLOW) return rc;
    double rows = 0;                    // a node's run calls give every shard the same rows
    if (gnuais_batch_info(nd->shards[0]->b, "rows", &rows) != GNUAIS_OK) return node_fail(GNUAIS_E_STATE, "node_drain_long_frames_unique: rows");
    const int pushed = h_first ? gnuais_long_uniq_push_heard_signal(nd->lq, nd->lq_frames.data(),
                                                                    measured ? nd->lq_signal.data() : nullptr, got,
                                                                    (long long) rows, h_out, h_copies, max, n_out, h_first,
                                                                    h_members, n_members)
                               : gnuais_long_uniq_push(nd->lq, nd->lq_frames.data(), got, (long long) rows, h_out, h_copies, max,
                                                       n_out);
    if (pushed != GNUAIS_OK) return node_fail(GNUAIS_E_ARG, "node_drain_long_frames_unique: the merge refused its input");
    return rc;              // GNUAIS_E_OVERFLOW of a device is reported with what was drained
}

int gnuais_node_drain_long_frames_unique(gnuais_node *nd, gnuais_long_frame *h_out, int32_t *h_copies, int max, int *n_out)
{
    if (!nd || !n_out || max < 0 || (max > 0 && (!h_out || !h_copies)))
        return node_fail(GNUAIS_E_ARG, "node_drain_long_frames_unique: argument");
    return node_drain_long_unique(nd, h_out, h_copies, max, n_out, nullptr, nullptr, nullptr);
}

int gnuais_node_drain_long_frames_heard(gnuais_node *nd, gnuais_long_frame *h_out, int32_t *h_copies, int max, int *n_out,
                                        int32_t *h_first, gnuais_hearer *h_members, int *n_members)
{
    if (!nd || !n_out || !n_members || !h_first || max < 0 || (max > 0 && (!h_out || !h_copies || !h_members)))
        return node_fail(GNUAIS_E_ARG, "node_drain_long_frames_heard: argument");
    *n_members = 0;
    h_first[0] = 0;
    return node_drain_long_unique(nd, h_out, h_copies, max, n_out, h_first, h_members, n_members);
}

// Streamed sentences of the whole node: gnuais_batch_stream_nmea() on every shard, each from its own thread.  Shard g's
// channels all lie before shard g+1's and a sentence does not name its channel (protodec.c:857-859: always 'A'), so the
// shards' texts written out in shard order are the node's sentences in the reference's order for that call.
int gnuais_node_stream_nmea(gnuais_node *nd, const char **texts, size_t *lens, int *n_sentences, int *n_frames)
{
    if (!nd || !texts || !lens) return node_fail(GNUAIS_E_ARG, "node_stream_nmea: NULL argument");
    std::vector<Shard *> &sh = nd->shards;
    std::vector<int> ns(sh.size(), 0), nf(sh.size(), -1);
    for (size_t i = 0; i < sh.size(); ++i) { texts[i] = nullptr; lens[i] = 0; }    // a shard that fails leaves nothing stale
    const int rc = run_all(nd, [&](Shard &s, size_t i) {
        return gnuais_batch_stream_nmea(s.b, &texts[i], &lens[i], &ns[i], &nf[i]);
    });
    int sent = 0, frames = 0;
    bool filling = false;
    for (size_t i = 0; i < sh.size(); ++i) {
        sent += ns[i];
        if (nf[i] < 0) filling = true; else frames += nf[i];
    }
    if (n_sentences) *n_sentences = sent;
    if (n_frames) *n_frames = filling ? -1 : frames;        // every shard fills and drains in the same call
    return rc;
}

int gnuais_node_discard_frames(gnuais_node *nd)
{
    if (!nd) return node_fail(GNUAIS_E_ARG, "node_discard_frames: NULL");
    return run_all(nd, [](Shard &s, size_t) { return gnuais_batch_discard_frames(s.b, nullptr); });
}

int gnuais_node_counters(gnuais_node *nd, gnuais_counters *h_out)
{
    if (!nd || !h_out) return node_fail(GNUAIS_E_ARG, "node_counters: argument");
    return run_all(nd, [&](Shard &s, size_t) { return gnuais_batch_counters(s.b, h_out + s.first); });
}

int gnuais_node_total_received(gnuais_node *nd, long long *total)
{
    if (!nd || !total) return node_fail(GNUAIS_E_ARG, "node_total_received: argument");
    std::vector<long long> t(nd->shards.size(), 0);
    const int rc = run_all(nd, [&](Shard &s, size_t i) { return gnuais_batch_total_received(s.b, &t[i]); });
    *total = 0;
    for (long long v : t) *total += v;
    return rc;
}

int gnuais_node_maxval(gnuais_node *nd, int16_t *h_out)
{
    if (!nd || !h_out) return node_fail(GNUAIS_E_ARG, "node_maxval: argument");
    return run_all(nd, [&](Shard &s, size_t) { return gnuais_batch_maxval(s.b, h_out + s.first); });
}

int gnuais_node_pll_state(gnuais_node *nd, gnuais_pll_state *h_out)
{
    if (!nd || !h_out) return node_fail(GNUAIS_E_ARG, "node_pll_state: argument");
    return run_all(nd, [&](Shard &s, size_t) { return gnuais_batch_pll_state(s.b, h_out + s.first); });
}

int gnuais_node_set_option(gnuais_node *nd, const char *name, int value)
{
    if (!nd || !name) return node_fail(GNUAIS_E_ARG, "node_set_option: argument");
    return run_all(nd, [&](Shard &s, size_t) { return gnuais_batch_set_option(s.b, name, value); });
}

int gnuais_node_autotune(gnuais_node *nd, const int16_t *const *d_samples, int len, void *const *streams,
                         float *best_ms_max)
{
    if (!nd || !d_samples) return node_fail(GNUAIS_E_ARG, "node_autotune: argument");
    std::vector<Shard *> &sh = nd->shards;
    std::vector<float> ms(sh.size(), 0.0f);
    // one device after the other: the measurement of one batch must not see another batch's host thread at work
    int rc = GNUAIS_OK;
    for (size_t i = 0; i < sh.size() && rc == GNUAIS_OK; ++i) {
        Shard *s = sh[i];
        s->w.submit([&, s, i] { return gnuais_batch_autotune(s->b, d_samples[i], len, streams ? streams[i] : nullptr, &ms[i]); });
        rc = s->w.wait();
        if (rc != GNUAIS_OK) g_node_err = s->w.err;
    }
    if (best_ms_max) *best_ms_max = *std::max_element(ms.begin(), ms.end());
    return rc;
}

} // extern "C"
