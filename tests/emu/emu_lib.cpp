/*
 * emu_lib.cpp — lane-lockstep CPU execution of the HIP kernels' source, for tests only.
 * Exposes: table build, the real host planner, and "launch" of the run / spectral kernels.
 */
#ifndef AACG_EMU_SCHEDULER
#define AACG_EMU_SCHEDULER              /* devport_emu.h: this translation unit has the schedule controller */
#endif
#include <atomic>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <memory>
#include <string>
#include <algorithm>
#include <vector>
#include <linux/futex.h>
#include <sys/syscall.h>
#include <unistd.h>

#include "../../aac.js_amd/csrc/aacg_kernels.h"
#include "../../aac.js_amd/csrc/aacg_parse.h"
#include "../../aac.js_amd/csrc/aacg_host.h"
#include "../../aac.js_amd/csrc/aacg_routes.h"
#include "emu_launch.h"

thread_local emu_lane_ctx g_emu;
int g_emu_fault_kind = EMU_FAULT_NONE, g_emu_fault_lo = 0, g_emu_fault_hi = 0, g_emu_fault_wave = -1;

namespace {

struct launch_arg {
    emu_lane_ctx ctx;
    const aacg_kparams* P;
    int kind;     /* 1 run kernel (key = its switches, aacg_routes.h), 2 spectral, 3/4 optional stages (quant / f32), 7 front end, 8/9 coupling passes */
    unsigned key;
    int n_units;
    const aacg_parse_params* PP;
    const aacg_couple_params* Q;
    const aacg_rv_args* V;
};

/* the run kernel with these switches: one case per registered kernel (aacg_run_kernels.h).  The non-temporal variants load through
 * the same emulated instruction, so AACG_RK_NT is dropped from the body's key; every kernel runs on the emulator's sixteen waves. */
void run_kernel(unsigned key, const aacg_kparams& P, const aacg_rv_args* V)
{
#define EMU_RUN_KERNEL(suffix, k, waves, args) case k: imdct_run_body<AACG_RUN_BODY_ARGS((k) & ~AACG_RK_NT)>(P, V); break;
#define EMU_RUN_KERNEL_SET(set, ROWS) ROWS(EMU_RUN_KERNEL)
    switch (key) {
    AACG_RUN_KERNEL_SETS(EMU_RUN_KERNEL_SET)
    default: std::abort();                          /* a route without a kernel */
    }
#undef EMU_RUN_KERNEL_SET
#undef EMU_RUN_KERNEL
}

void sched_lane_enter();
void sched_lane_done();
struct emu_abort {};                       /* thrown through the kernel source by a lane whose decode has ended in a deadlock report */

void lane_body(launch_arg* a);
void* lane_main(void* p)
{
    launch_arg* a = (launch_arg*)p;
    g_emu = a->ctx;
    if (!g_emu.w->sw) { lane_body(a); return nullptr; }
    try {
        sched_lane_enter();
        lane_body(a);
        sched_lane_done();
    } catch (const emu_abort&) {}
    return nullptr;
}

void lane_body(launch_arg* a)
{
    if (a->kind == 7) aacg_parse::parse_body(*a->PP);
    else if (a->kind == 1) run_kernel(a->key, *a->P, a->V);
    else if (a->kind == 8) couple_spec_body(*a->Q, 4);
    else if (a->kind == 9) couple_pcm_body(*a->Q, 4);
    else if (a->kind == 3) spectral_ex_body<AACG_INPUT_QUANT_I16>(*a->P, a->n_units);
    else if (a->kind == 4) spectral_ex_body<AACG_INPUT_SPEC_F32>(*a->P, a->n_units);
    else if (a->kind == 10) tns_matrices_body(a->P->tns, (double*)(void*)a->P->scratch, (uint32_t)a->n_units);
    else                   spectral_body(*a->P, a->n_units);
}

int g_out_kind = AACG_OUTPUT_F32;          /* emu_set_output_kind: the next decodes store int16 PCM */
int g_unfused = 0;                         /* emu_set_unfused: independent coupling as the separate pass over the PCM even where the engine fuses it */
int g_rv = 1;                              /* emu_set_rv: chains longer than a run through the run-to-run rendezvous (the engine's route; 2: blocks in reverse); 0: recomputed frames */
int g_staged = 0;                          /* emu_set_staged: optional stages as a launch of their own even where the engine would not */
int g_pipelined = 0;                       /* emu_set_pipelined: the route aacg_decode_pipelined takes for the plan, as one launch */
std::string g_err;
std::vector<unsigned> g_keys;              /* emu_last_keys: the run kernels (AACG_RK_* keys, NT bit included) the last decode launched, in order */

/* ------------------------------------------------------------------------------------------------------------------------ */
/* Schedule-controlled mode (see devport_emu.h): one wave runs at a time, a controller picks the next one by a policy           */
/* ------------------------------------------------------------------------------------------------------------------------ */
enum { POL_OFF, POL_NATURAL, POL_REVERSED, POL_STRAGGLER, POL_SPRINTER, POL_RANDOM, POL_CELL };
struct sched_cfg { int policy = POL_OFF, a = 0, b = 0; unsigned seed = 0; int span = 0; } g_cfg;     /* emu_set_schedule */
long g_steps = 0;                          /* emu_sched_steps: turns the controller granted in the last decode */
std::vector<long long> g_trace;            /* emu_sched_trace: the wave (launch, workgroup, wave as one number) of every turn of the last decode */
int g_last_links = 0, g_last_chains = 0;   /* emu_sched_cells: in-launch cells / chains (= cross-launch cells per launch boundary) of the last decode's plan */
bool g_sched_failed = false;               /* a launch of this decode ended in a deadlock report (g_err) */
const int EMU_ERR_DEADLOCK = -9001;
/* policy `cell`: the one rendezvous state word whose two sides the controller orders; side 0 publishes tails, side 1 a head */
struct watch_cfg { const void* addr = nullptr; int variant = 0; int launch[2] = {0, 0}, wg[2] = {-1, -1}; } g_watch;

}  // namespace

struct lane_rec { int kind; const void* addr; long long val; bool parked, go; };     /* a lane at a scheduling point: which, on what, for which value */

struct emu_sched_wave {
    std::atomic<int> state{0};             /* low 16 bits: lanes running; high 16: lanes waiting in the wave's barrier */
    std::atomic<int> gen{0};               /* the barrier's generation: the futex word its waiters sleep on */
    int parked = 64, alive = 64;           /* lanes at a scheduling point / that have not returned (controller's mutex) */
    int launch = 0, wg = 0, wave = 0;
    long long key = 0;                     /* (launch, workgroup, wave) as one number: the natural order */
    double prio = 0;                       /* policy random */
    emu_block* blk = nullptr;
    pthread_cond_t cv;
    lane_rec lane[64];
};

namespace {

struct sched_wg {
    emu_block blk;
    std::vector<emu_wave> wv;
    std::vector<emu_sched_wave> sw;
    std::vector<launch_arg> args;
    std::vector<pthread_t> tid;
};
struct sched_state {
    pthread_mutex_t mu = PTHREAD_MUTEX_INITIALIZER;
    pthread_cond_t main_cv = PTHREAD_COND_INITIALIZER;
    std::vector<std::unique_ptr<sched_wg>> wgs;
    std::function<void()> progress;        /* starts the launches that may start now (mutex held) */
    std::vector<int> waves_left;           /* per launch: waves that have not finished */
    bool done = false;
    std::atomic<bool> abort{false};
    std::string report;
    long steps = 0;
    std::vector<long long> trace;
    sched_cfg cfg;
    uint32_t rng = 1;
    std::vector<long> changes;             /* policy random: the turns at which the wave about to run drops below all others */
    size_t n_changed = 0;
    watch_cfg watch;
    bool loaded[2] = {false, false}, swapped[2] = {false, false}, at_cas[2] = {false, false};
    emu_sched_wave* loader[2] = {nullptr, nullptr};
};
sched_state* g_s = nullptr;

uint32_t sched_rand(sched_state& s) { s.rng ^= s.rng << 13; s.rng ^= s.rng >> 17; s.rng ^= s.rng << 5; return s.rng; }

void futex_wake_all(std::atomic<int>* w) { syscall(SYS_futex, (int*)w, FUTEX_WAKE_PRIVATE, INT_MAX, nullptr, nullptr, 0); }

int side_of(const sched_state& s, const emu_sched_wave* w)
{
    for (int i = 0; i < 2; i++)
        if (s.watch.launch[i] == w->launch && (s.watch.wg[i] < 0 || s.watch.wg[i] == w->wg)) return i;
    return -1;
}

/* may this parked lane go on?  Its own condition (a flag's value, the workgroup's barrier), then the holds of policy `cell` */
bool lane_ready(const sched_state& s, const emu_sched_wave* w, const lane_rec& L, bool* held = nullptr)
{
    if (L.kind == EMU_SP_FLAG_WAIT && __atomic_load_n((const int*)L.addr, __ATOMIC_ACQUIRE) != (int)L.val) return false;
    if (L.kind == EMU_SP_FLAG_WAIT_GE && __atomic_load_n((const int*)L.addr, __ATOMIC_ACQUIRE) < (int)L.val) return false;
    if (L.kind == EMU_SP_BLOCK_SYNC && w->blk->sync_gen == (int)L.val) return false;
    if (!s.watch.addr) return true;
    const int sd = side_of(s, w);
    if (sd < 0) return true;
    const bool on = L.addr == s.watch.addr, load = on && L.kind == EMU_SP_G_LOAD_U64, cas = on && L.kind == EMU_SP_G_CAS;
    const int P = 0, C = 1;
    bool hold = false;
    switch (s.watch.variant) {
    case 1: hold = (sd == C && s.loader[C] == w && !s.swapped[P]) || (sd == P && cas && !s.loaded[C]); break;   /* both load, the publisher swaps first */
    case 2: hold = (sd == P && s.loader[P] == w && !s.swapped[C]) || (sd == C && cas && !s.loaded[P]); break;   /* both load, the consumer swaps first */
    case 3: hold = (sd == P && cas && !s.swapped[C]) || (sd == C && load && !s.at_cas[P]); break;  /* the consumer's whole visit between the publisher's payload and its swap */
    case 4: hold = sd == C && load && !s.swapped[P]; break;                                          /* the publisher's visit, then the consumer's */
    case 5: hold = sd == P && load && !s.swapped[C]; break;                                          /* the consumer's visit, then the publisher's */
    }
    if (hold && held) *held = true;
    return !hold;
}

double score_of(const sched_state& s, const emu_sched_wave* w)
{
    switch (s.cfg.policy) {
    case POL_REVERSED:  return (double)w->key;
    case POL_STRAGGLER: return (w->wave == s.cfg.a ? -1e15 : 0.0) - (double)w->key;
    case POL_SPRINTER:  return (w->wave == s.cfg.a ? 1e15 : 0.0) - (double)w->key;
    case POL_RANDOM:    return w->prio;
    default:            return -(double)w->key;
    }
}

const char* sp_name(int kind)
{
    static const char* n[] = {"a skipped wait", "dp_flag_set", "dp_flag_wait", "dp_flag_wait_ge", "dp_block_sync", "dp_g_load_u64", "dp_g_cas_u64", "dp_g_store", "dp_g_load", "dp_vm_drain"};
    return n[kind];
}

/* nobody can run and not everybody has finished: who waits for what */
std::string deadlock_report(const sched_state& s)
{
    std::string r = "deadlock under the forced schedule: no wave is runnable.";
    char line[320];
    for (auto& wg : s.wgs)
        for (auto& w : wg->sw) {
            if (!w.alive) continue;
            int shown = 0;
            for (int l = 0; l < 64; l++) {
                const lane_rec& L = w.lane[l];
                if (!L.parked) continue;
                bool dup = false;
                for (int m = 0; m < l && !dup; m++) dup = w.lane[m].parked && w.lane[m].kind == L.kind && w.lane[m].addr == L.addr && w.lane[m].val == L.val;
                if (dup || shown++ >= 4) continue;
                if (L.kind == EMU_SP_FLAG_WAIT || L.kind == EMU_SP_FLAG_WAIT_GE) {
                    const long off = (long)((const unsigned char*)L.addr - w.blk->lds);
                    /* the run body's flags: [task] = "my tails are in my slot" (the next task waits for it), [AACG_WG_WAVES + task] =
                     * "I have read the previous frame's slot" (task + AACG_HALF_SLOTS - 1 waits for it) */
                    const int idx = w.blk->flags_off >= 0 ? (int)(off - w.blk->flags_off) / 4 : -1;
                    const int task = idx < 0 ? -1 : idx < AACG_WG_WAVES ? idx + 1 : idx - AACG_WG_WAVES + AACG_HALF_SLOTS - 1;
                    bool held = false;
                    const bool ok = lane_ready(s, &w, L, &held);
                    std::snprintf(line, sizeof line, " [launch %d workgroup %d wave %d task %d: %s on the flag at LDS byte %ld (flags[%d]) for value %s%lld, it holds %d%s]",
                                  w.launch, w.wg, w.wave, task, sp_name(L.kind), off, idx, L.kind == EMU_SP_FLAG_WAIT_GE ? ">= " : "", L.val,
                                  __atomic_load_n((const int*)L.addr, __ATOMIC_ACQUIRE), ok ? "" : held ? "; held by the cell schedule" : "");
                } else if (L.kind == EMU_SP_BLOCK_SYNC) {
                    std::snprintf(line, sizeof line, " [launch %d workgroup %d wave %d: in dp_block_sync with %d of %d lanes of the workgroup]",
                                  w.launch, w.wg, w.wave, w.blk->sync_arrived, w.blk->threads);
                } else {
                    std::snprintf(line, sizeof line, " [launch %d workgroup %d wave %d: held by the cell schedule at %s]", w.launch, w.wg, w.wave, sp_name(L.kind));
                }
                r += line;
            }
        }
    return r;
}

/* the wave that had the turn has no running lane left (mutex held): give the turn to the best runnable wave */
void sched_pick()
{
    sched_state& s = *g_s;
    for (;;) {
        if (s.progress) s.progress();
        emu_sched_wave* best = nullptr;
        double best_score = 0;
        int unfinished = 0;
        for (auto& wg : s.wgs)
            for (auto& w : wg->sw) {
                if (!w.alive) continue;
                unfinished++;
                if (!w.parked) continue;
                bool ready = false;
                for (int l = 0; l < 64 && !ready; l++) ready = w.lane[l].parked && lane_ready(s, &w, w.lane[l]);
                if (!ready) continue;
                const double sc = score_of(s, &w);
                if (!best || sc > best_score || (sc == best_score && w.key < best->key)) { best = &w; best_score = sc; }
            }
        if (!best) {
            if (!unfinished) s.done = true;
            else {
                s.report = deadlock_report(s);
                s.abort.store(true);
                for (auto& wg : s.wgs)
                    for (auto& w : wg->sw) { pthread_cond_broadcast(&w.cv); w.gen.fetch_add(1); futex_wake_all(&w.gen); }
            }
            pthread_cond_signal(&s.main_cv);
            return;
        }
        if (s.cfg.policy == POL_RANDOM && s.n_changed < s.changes.size() && s.steps >= s.changes[s.n_changed]) {
            best->prio = -(double)(1 + s.n_changed++);      /* probabilistic concurrency testing: the wave about to run falls behind everybody */
            continue;
        }
        int n = 0;
        for (int l = 0; l < 64; l++) {
            lane_rec& L = best->lane[l];
            if (L.parked && lane_ready(s, best, L)) { L.parked = false; L.go = true; n++; }
        }
        best->parked -= n;
        best->state.fetch_add(n);
        s.steps++;
        s.trace.push_back(best->key);
        pthread_cond_broadcast(&best->cv);
        return;
    }
}

void sched_wait_go(sched_state& s, emu_sched_wave* w, lane_rec& L)
{
    while (!L.go && !s.abort.load()) pthread_cond_wait(&w->cv, &s.mu);
    const bool go = L.go;
    L.go = false;
    pthread_mutex_unlock(&s.mu);
    if (!go) throw emu_abort();
}

void sched_lane_enter()                      /* a lane's first step: created parked, it waits for its wave's first turn */
{
    sched_state& s = *g_s;
    emu_sched_wave* w = g_emu.w->sw;
    pthread_mutex_lock(&s.mu);
    sched_wait_go(s, w, w->lane[g_emu.lane]);
}

void sched_lane_done()
{
    sched_state& s = *g_s;
    emu_sched_wave* w = g_emu.w->sw;
    pthread_mutex_lock(&s.mu);
    if (--w->alive == 0) s.waves_left[(size_t)w->launch]--;
    if ((w->state.fetch_sub(1) & 0xffff) == 1) sched_pick();
    pthread_mutex_unlock(&s.mu);
}

/* a workgroup joins the resident set: its lanes are created parked (mutex held, or before the controller starts) */
void sched_add_wg(sched_state& s, int launch, const aacg_kparams* P, unsigned key, int block, int waves, size_t lds_bytes, const aacg_rv_args* V)
{
    s.wgs.emplace_back(new sched_wg);
    sched_wg& g = *s.wgs.back();
    const int threads = waves * 64;
    g.wv = std::vector<emu_wave>((size_t)waves);
    g.sw = std::vector<emu_sched_wave>((size_t)waves);
    g.args.resize((size_t)threads);
    g.tid.resize((size_t)threads);
    g.blk.lds = (unsigned char*)aligned_alloc(512, (lds_bytes + 511) & ~(size_t)511);
    g.blk.lds_bytes = lds_bytes;
    g.blk.block_id = block;
    g.blk.threads = threads; g.blk.sync_arrived = 0; g.blk.sync_gen = 0; g.blk.flags_off = -1;
    std::memset(g.blk.lds, 0xff, lds_bytes);
    if ((size_t)launch >= s.waves_left.size()) s.waves_left.resize((size_t)launch + 1, 0);
    s.waves_left[(size_t)launch] += waves;
    for (int w = 0; w < waves; w++) {
        emu_sched_wave& sw = g.sw[(size_t)w];
        sw.launch = launch; sw.wg = block; sw.wave = w; sw.blk = &g.blk;
        sw.key = ((long long)launch * 4096 + block) * 64 + w;
        sw.prio = (double)(64 + (sched_rand(s) & 0xfffffu));
        pthread_cond_init(&sw.cv, nullptr);
        for (int l = 0; l < 64; l++) sw.lane[l] = lane_rec{EMU_SP_NONE, nullptr, 0, true, false};
        g.wv[(size_t)w].sw = &sw;
    }
    pthread_attr_t attr;
    pthread_attr_init(&attr);
    pthread_attr_setstacksize(&attr, 256 * 1024);
    for (int t = 0; t < threads; t++) {
        launch_arg& a = g.args[(size_t)t];
        a.ctx = emu_lane_ctx{t & 63, t >> 6, &g.wv[(size_t)(t >> 6)], &g.blk};
        a.P = P; a.kind = 1; a.key = key; a.n_units = 0; a.PP = nullptr; a.Q = nullptr; a.V = V;
        if (pthread_create(&g.tid[(size_t)t], &attr, lane_main, &a)) { std::fprintf(stderr, "emu: cannot create lane thread %d\n", t); std::abort(); }
    }
    pthread_attr_destroy(&attr);
}

void sched_init(sched_state& s)
{
    g_s = &s;
    s.cfg = g_cfg;
    s.watch = g_cfg.policy == POL_CELL ? g_watch : watch_cfg();
    s.rng = g_cfg.seed * 2654435761u + 0x9e3779b9u;
    if (!s.rng) s.rng = 1;
    if (g_cfg.policy == POL_RANDOM) {
        const int span = g_cfg.span > 1 ? g_cfg.span : 2048;
        for (int i = 0; i < g_cfg.b; i++) s.changes.push_back(1 + (long)(sched_rand(s) % (uint32_t)(span - 1)));
        std::sort(s.changes.begin(), s.changes.end());
    }
}

/* runs everything that was added (and what `progress` adds on the way) to the end or to a deadlock report */
int sched_run(sched_state& s)
{
    pthread_mutex_lock(&s.mu);
    sched_pick();
    while (!s.done && !s.abort.load()) pthread_cond_wait(&s.main_cv, &s.mu);
    pthread_mutex_unlock(&s.mu);
    for (auto& wg : s.wgs) {
        for (pthread_t t : wg->tid) pthread_join(t, nullptr);
        for (auto& w : wg->sw) pthread_cond_destroy(&w.cv);
        free(wg->blk.lds);
    }
    g_s = nullptr;
    g_steps += s.steps;
    g_trace.insert(g_trace.end(), s.trace.begin(), s.trace.end());
    if (s.abort.load()) { g_err = s.report; g_sched_failed = true; return EMU_ERR_DEADLOCK; }
    return 0;
}

}  // namespace

void emu_sched_wave_barrier()
{
    emu_sched_wave* w = g_emu.w->sw;
    const int my = w->gen.load();
    const int old = w->state.fetch_add((1 << 16) - 1);          /* one lane fewer running, one more in the barrier: one step */
    if ((old >> 16) == 63) {                                     /* the last of the wave: everybody runs on */
        w->state.store(64);
        w->gen.fetch_add(1);
        futex_wake_all(&w->gen);
        return;
    }
    if ((old & 0xffff) == 1) {                                   /* the last running lane; the others are parked or here: the turn goes on */
        pthread_mutex_lock(&g_s->mu);
        sched_pick();
        pthread_mutex_unlock(&g_s->mu);
    }
    while (w->gen.load() == my) syscall(SYS_futex, (int*)&w->gen, FUTEX_WAIT_PRIVATE, my, nullptr, nullptr, 0);
    if (g_s->abort.load()) throw emu_abort();
}

void emu_sched_point(int kind, const void* addr, long long val)
{
    sched_state& s = *g_s;
    emu_sched_wave* w = g_emu.w->sw;
    pthread_mutex_lock(&s.mu);
    lane_rec& L = w->lane[g_emu.lane];
    if (kind == EMU_SP_BLOCK_SYNC) {                             /* the barrier opens when the workgroup's last lane is here; every lane still waits for its wave's turn */
        val = w->blk->sync_gen;
        if (++w->blk->sync_arrived == w->blk->threads) { w->blk->sync_arrived = 0; w->blk->sync_gen++; }
    }
    if (kind == EMU_SP_FLAG_SET && w->blk->flags_off < 0)        /* a wave's first flag is flags[wave] */
        w->blk->flags_off = (int)((const unsigned char*)addr - w->blk->lds) - 4 * w->wave;
    if (kind == EMU_SP_G_CAS && addr == s.watch.addr) { const int sd = side_of(s, w); if (sd >= 0) s.at_cas[sd] = true; }
    L = lane_rec{kind, addr, val, true, false};
    w->parked++;
    if ((w->state.fetch_sub(1) & 0xffff) == 1) sched_pick();
    sched_wait_go(s, w, L);
}

void emu_sched_note(int kind, const void* addr)
{
    sched_state& s = *g_s;
    /* lane 0's load is the one the wave goes by (dp_first_u64), and lane 0 swaps: the other lanes may have run ahead of a
     * dp_flag_set that lane 0 alone executes, so their loads say nothing about when the wave looked */
    if (addr != s.watch.addr || g_emu.lane != 0) return;
    emu_sched_wave* w = g_emu.w->sw;
    pthread_mutex_lock(&s.mu);
    const int sd = side_of(s, w);
    if (sd >= 0) {
        if (kind == EMU_SP_G_LOAD_U64) { s.loaded[sd] = true; s.loader[sd] = w; }
        else s.swapped[sd] = true;
    }
    pthread_mutex_unlock(&s.mu);
}

namespace {

/* one workgroup of a launch, its lanes as threads (emu_launch.h): no schedule controller, so lane_body without lane_main's turn-taking */
void run_block(const aacg_kparams& P, int kind, unsigned key, int block, int waves, size_t lds_bytes, int n_units = 0, const aacg_parse_params* PP = nullptr,
               const aacg_couple_params* Q = nullptr, const aacg_rv_args* V = nullptr)
{
    launch_arg a{};
    a.P = &P; a.kind = kind; a.key = key; a.n_units = n_units; a.PP = PP; a.Q = Q; a.V = V;
    auto body = [&] { lane_body(&a); };
    emu_launch_block(block, waves * 64, lds_bytes, body);
}

/* a whole grid, workgroup after workgroup */
void launch(const aacg_kparams& P, int kind, unsigned key, int grid, int waves, size_t lds_bytes, int n_units = 0, const aacg_parse_params* PP = nullptr,
            const aacg_couple_params* Q = nullptr, const aacg_rv_args* V = nullptr)
{
    if (kind == 1) g_keys.push_back(key);
    if (kind == 1 && g_cfg.policy != POL_OFF) {
        /* schedule-controlled mode: the workgroups of a run kernel's launch are resident together, one set of waves under one controller */
        if (g_sched_failed) return;
        sched_state s;
        sched_init(s);
        for (int b = 0; b < grid; b++) sched_add_wg(s, 0, &P, key, b, waves, lds_bytes, V);
        sched_run(s);
        return;
    }
    for (int b = 0; b < grid; b++) run_block(P, kind, key, b, waves, lds_bytes, n_units, PP, Q, V);
}

size_t run_lds_bytes(unsigned key)
{
    const bool quant = (key & AACG_RK_QUANT) != 0;
    if (key & AACG_RK_EX) return quant ? AACG_LDS_BYTES_QUANT_EX : AACG_LDS_BYTES_F32_EX;
    return quant ? AACG_LDS_BYTES_QUANT : AACG_LDS_BYTES_F32;
}

aacg_tables g_tab;
int g_tab_index = -1;

}  // namespace

extern "C" {

const char* emu_last_error() { return g_err.c_str(); }
void emu_set_staged(int on) { g_staged = on; }
void emu_set_pipelined(int on) { g_pipelined = on; }
/* the keys of the run kernels the last emu_decode* launched (a coupling elements' pass included), in launch order: how many there
 * were; the first `cap` of them into `keys` */
int emu_last_keys(unsigned* keys, int cap)
{
    for (int i = 0; i < cap && i < (int)g_keys.size(); i++) keys[i] = g_keys[(size_t)i];
    return (int)g_keys.size();
}
void emu_set_rv(int on) { g_rv = on; }
/* Schedule-controlled mode for the run kernels of later decodes (devport_emu.h).  policy: 0 off (the default: lanes as the OS
 * schedules them, workgroup after workgroup), 1 natural (lowest launch, workgroup, wave first), 2 reversed (highest first),
 * 3 straggler(a) (wave a of every workgroup only when nobody else can run), 4 sprinter(a) (wave a first whenever it can run),
 * 5 random (seeded priorities per wave, b times the wave about to run drops behind all others, at turns drawn from
 * [1, span): span = the turns of a run of the same decode, emu_sched_steps), 6 cell(a, b): natural, and at rendezvous cell a
 * (emu_decode: the in-launch cell with that link number; emu_decode_pipelined: chain a % chains between launches a / chains
 * and the next; emu_sched_cells gives the counts) the two sides in order b = 1: both load the state word, the publisher
 * swaps first; 2: both load, the consumer swaps first; 3: the consumer's whole visit between the publisher's payload stores
 * and its swap; 4: publisher, then consumer; 5: consumer, then publisher. */
void emu_set_schedule(int policy, int a, int b, unsigned seed, int span) { g_cfg.policy = policy; g_cfg.a = a; g_cfg.b = b; g_cfg.seed = seed; g_cfg.span = span; }
long emu_sched_steps() { return g_steps; }
/* which wave had each turn of the last decode, ((launch * 4096 + workgroup) * 64 + wave): how many; the first `cap` into `out` */
int emu_sched_trace(long long* out, int cap)
{
    for (int i = 0; i < cap && i < (int)g_trace.size(); i++) out[i] = g_trace[(size_t)i];
    return (int)g_trace.size();
}
void emu_sched_cells(int* links, int* chains) { *links = g_last_links; *chains = g_last_chains; }
/* Breaks an emulated primitive on purpose, so that a test can show it would see the broken hand-off (kinds: EMU_FAULT_* of
 * devport_emu.h; 1 skip_wait, 2 early_set and 4 lost_set: flags in LDS bytes [lo, hi), early_set for waiting wave `wave` only;
 * 3 blind_cas; 0 none, the default) */
void emu_set_fault(int kind, int lo, int hi, int wave) { g_emu_fault_kind = kind; g_emu_fault_lo = lo; g_emu_fault_hi = hi; g_emu_fault_wave = wave; }
/* where the run body's flags begin in its LDS, in bytes: behind the tables (quant: the dequantisation part too; the eight-wave
 * body keeps a shorter IQ table) and the slots */
int emu_flags_offset(int quant, int half)
{
    const int tab = !quant ? AACG_TAB_F32_FLOATS : half ? AACG_TAB_QUANT_FLOATS - AACG_TAB_IQ_CUT(AACG_HALF_IQH) : AACG_TAB_QUANT_FLOATS;
    return 4 * (AACG_TAB_SLOT_BASE(tab) + (half ? AACG_HALF_SLOTS : AACG_WG_WAVES) * AACG_SLOT_FLOATS);
}
void emu_set_unfused(int on) { g_unfused = on; }
void emu_set_output_kind(int kind) { g_out_kind = kind; }       /* AACG_OUTPUT_*: the pcm buffer of later decodes is int16 */

int emu_get_windows(int sample_index, float* dst /* 1024+1024+128+128 */)
{
    aacg_tables t; aacg_host_windows w;
    int rc = aacg_build_tables(sample_index, &t, &w);
    if (rc) return rc;
    std::memcpy(dst, w.sine_long, 4096); std::memcpy(dst + 1024, w.kbd_long, 4096);
    std::memcpy(dst + 2048, w.sine_short, 512); std::memcpy(dst + 2176, w.kbd_short, 512);
    return 0;
}

int emu_get_iq_sf(float* iq /* 8192 */, float* sf /* 428 */)
{
    aacg_tables t;
    int rc = aacg_build_tables(3, &t, nullptr);
    if (rc) return rc;
    std::memcpy(iq, t.iq, sizeof t.iq); std::memcpy(sf, t.sf, 428 * 4);
    return 0;
}

/* plan only: returns number of runs (or <0); fills counts for inspection */
int emu_plan(const aacg_unit_desc* units, uint32_t n_units, int sample_index, int max_streams, int max_channels,
             const uint8_t* parity, aacg_run* runs_out, uint32_t runs_cap, int32_t* info /* zero_fill, n_chains, coef_blocks, meta_blocks */)
{
    aacg_plan_host ph;
    int rc = aacg_plan_build(units, n_units, sample_index, max_streams, max_channels, parity, &ph, &g_err);
    if (rc) return rc;
    if (runs_out) for (size_t i = 0; i < ph.runs.size() && i < runs_cap; i++) runs_out[i] = ph.runs[i];
    if (info) { info[0] = ph.zero_fill; info[1] = (int32_t)ph.chains.size(); info[2] = (int32_t)ph.coef_blocks; info[3] = (int32_t)ph.meta_blocks; }
    return (int)ph.runs.size();
}

/* host planner only: a plan for `first`, then aacg_plan_refresh_host with `next` (tns_spec: the engine's TNS mode) */
int emu_plan_refresh(const aacg_unit_desc* first, const aacg_unit_desc* next, uint32_t n_units, int sample_index, int max_streams,
                     int max_channels, int tns_spec)
{
    aacg_plan_host ph;
    std::vector<uint8_t> parity((size_t)max_streams * (size_t)max_channels, 0);
    int rc = aacg_plan_build(first, n_units, sample_index, max_streams, max_channels, parity.data(), &ph, &g_err);
    if (rc) return rc;
    return aacg_plan_refresh_host(&ph, next, n_units, sample_index, tns_spec != 0, &g_err);
}

/* full path: plan + "launch".  overlap_pool: [max_streams][max_channels][AACG_OV_BUFFERS][1024]; parity: [max_streams*max_channels] (0..AACG_OV_BUFFERS-1), updated. */
int emu_decode_tns(int input_kind, int sample_index, int max_streams, int max_channels,
                   const aacg_unit_desc* units, uint32_t n_units, const void* coeffs, const aacg_band_meta* meta,
                   const aacg_tns_info* tns, uint32_t n_tns,
                   float* pcm, size_t n_pcm_floats, float* overlap_pool, uint8_t* parity);
int emu_decode_ex(int input_kind, int sample_index, int max_streams, int max_channels,
                  const aacg_unit_desc* units, uint32_t n_units, const void* coeffs, const aacg_band_meta* meta,
                  const aacg_tns_info* tns, uint32_t n_tns, int pns_mode,
                  float* pcm, size_t n_pcm_floats, float* overlap_pool, uint8_t* parity);
int emu_decode_cce(int input_kind, int sample_index, int max_streams, int max_channels,
                   const aacg_unit_desc* units, uint32_t n_units, const void* coeffs, const aacg_band_meta* meta,
                   const aacg_tns_info* tns, uint32_t n_tns, int pns_mode, const aacg_cce_info* cce, uint32_t n_cce,
                   float* pcm, size_t n_pcm_floats, float* overlap_pool, uint8_t* parity);

int emu_decode(int input_kind, int sample_index, int max_streams, int max_channels,
               const aacg_unit_desc* units, uint32_t n_units, const void* coeffs, const aacg_band_meta* meta,
               float* pcm, size_t n_pcm_floats, float* overlap_pool, uint8_t* parity)
{
    return emu_decode_tns(input_kind, sample_index, max_streams, max_channels, units, n_units, coeffs, meta,
                          nullptr, 0, pcm, n_pcm_floats, overlap_pool, parity);
}

/* tns != NULL: AACG_TNS_SPEC */
int emu_decode_tns(int input_kind, int sample_index, int max_streams, int max_channels,
                   const aacg_unit_desc* units, uint32_t n_units, const void* coeffs, const aacg_band_meta* meta,
                   const aacg_tns_info* tns, uint32_t n_tns,
                   float* pcm, size_t n_pcm_floats, float* overlap_pool, uint8_t* parity)
{
    return emu_decode_ex(input_kind, sample_index, max_streams, max_channels, units, n_units, coeffs, meta, tns, n_tns,
                         AACG_PNS_REFERENCE, pcm, n_pcm_floats, overlap_pool, parity);
}

int emu_decode_ex(int input_kind, int sample_index, int max_streams, int max_channels,
                  const aacg_unit_desc* units, uint32_t n_units, const void* coeffs, const aacg_band_meta* meta,
                  const aacg_tns_info* tns, uint32_t n_tns, int pns_mode,
                  float* pcm, size_t n_pcm_floats, float* overlap_pool, uint8_t* parity)
{
    return emu_decode_cce(input_kind, sample_index, max_streams, max_channels, units, n_units, coeffs, meta, tns, n_tns, pns_mode,
                          nullptr, 0, pcm, n_pcm_floats, overlap_pool, parity);
}

/* pns_mode == AACG_PNS_SPEC: batches with AACG_UNIT_HAS_PNS units take the optional-stage routes;
 * cce != NULL: AACG_CCE_SPEC.  The route is the engine's: aacg_pick_route (aacg_routes.cpp), executed here as launch_run
 * (aacg_engine.hip) executes it. */
int emu_decode_cce(int input_kind, int sample_index, int max_streams, int max_channels,
                   const aacg_unit_desc* units, uint32_t n_units, const void* coeffs, const aacg_band_meta* meta,
                   const aacg_tns_info* tns, uint32_t n_tns, int pns_mode, const aacg_cce_info* cce, uint32_t n_cce,
                   float* pcm, size_t n_pcm_floats, float* overlap_pool, uint8_t* parity)
{
    if (g_tab_index != sample_index) { int rc = aacg_build_tables(sample_index, &g_tab, nullptr); if (rc) return rc; g_tab_index = sample_index; }
    aacg_plan_host ph;
    int rc = aacg_plan_build(units, n_units, sample_index, max_streams, max_channels, parity, &ph, &g_err, tns, n_tns, cce, n_cce);
    if (rc) return rc;
    g_keys.clear();
    g_steps = 0; g_trace.clear(); g_sched_failed = false; g_watch = watch_cfg();
    g_last_links = (int)ph.n_links_rv; g_last_chains = (int)ph.chains.size();
    if (ph.pcm_floats > n_pcm_floats) { g_err = "pcm buffer too small"; return AACG_ERR_CAPACITY; }
    if (ph.zero_fill) std::memset(pcm, 0, n_pcm_floats * (g_out_kind == AACG_OUTPUT_I16 ? 2 : 4));
    if (ph.any_pns && (pns_mode != AACG_PNS_SPEC || input_kind != AACG_INPUT_QUANT_I16)) { g_err = "PNS unit in a batch without AACG_PNS_SPEC"; return AACG_ERR_UNSUPPORTED; }
    aacg_route R = aacg_pick_route(input_kind, g_out_kind, (g_unfused ? AACG_DEBUG_ROUTE_UNFUSED_COUPLING : 0) | (g_rv ? 0 : AACG_DEBUG_ROUTE_RECOMPUTE), false, ph, g_pipelined != 0);
    if (g_staged && R.has_run && (R.run_key & AACG_RK_EX)) {     /* test switch: the optional stages as a launch of their own even where the engine runs them inside */
        R.stage = AACG_STAGE_SPECTRAL_EX; R.stage_quant = input_kind == AACG_INPUT_QUANT_I16;
        R.run_key = ph.needs_scratch ? AACG_RK_DD : 0; R.rv = false;
    }
    aacg_kparams P;
    std::memset(&P, 0, sizeof P);
    P.units = ph.units.data(); P.runs = ph.runs.data(); P.coeffs = coeffs; P.meta = meta; P.pcm = pcm;
    P.overlap = overlap_pool; P.tab = &g_tab; P.flip = 0; P.n_runs = (int32_t)ph.runs.size();
    P.tns = ph.any_tns ? ph.tns.data() : nullptr;
    std::vector<float> scratch(ph.needs_scratch ? ph.runs.size() * AACG_SLOT_FLOATS : 1, 0.0f);
    P.scratch = ph.needs_scratch ? scratch.data() : nullptr;
    /* the plan's TNS transition matrices, made once by a kernel of their own (aacg_tns_matrices): what the engine does when it
     * creates the plan; they ride in `scratch` for the launches that run filters (aacg_set_tns_m) */
    std::vector<double> tns_m(ph.any_tns ? ph.tns.size() * AACG_TNS_M_DOUBLES : 1, std::numeric_limits<double>::quiet_NaN());
    if (ph.any_tns) {
        aacg_kparams T = P;
        aacg_set_tns_m(&T, tns_m.data());
        launch(T, 10, 0, (int)((ph.tns.size() + AACG_WG_WAVES - 1) / AACG_WG_WAVES), AACG_WG_WAVES, 64, (int)ph.tns.size());
    }
    std::vector<float> spec;
    static aacg_pns_tables pns_tab;
    aacg_build_pns_tables(sample_index, &pns_tab);
    std::vector<float> side((size_t)ph.side_blocks * 1024u + 1, 0.0f);
    const int unit_blocks = (int)((n_units + AACG_WG_WAVES - 1) / AACG_WG_WAVES);
    auto couple = [&](int point) {
        for (uint32_t r = 0; r < ph.couple_rounds; r++) {
            const uint32_t first = ph.couple_first[(size_t)point * ph.couple_rounds + r], last = ph.couple_first[(size_t)point * ph.couple_rounds + r + 1];
            if (last <= first) continue;
            aacg_couple_params Q;
            Q.jobs = ph.couple_jobs.data() + first; Q.n_jobs = (int32_t)(last - first); Q.units = ph.units.data(); Q.meta = meta; Q.tab = &g_tab;
            Q.gains = ph.gains.data(); Q.spec = spec.data(); Q.side = side.data(); Q.pcm = pcm; Q.reserved = 0;
            launch(P, point == AACG_CCE_AFTER_IMDCT ? 9 : 8, 0, (Q.n_jobs + 3) / 4, 4, 64, 0, nullptr, &Q);
        }
    };
    if (R.rv) {
        /* plain batches with a chain longer than a run: every run 16 frames, a rendezvous between consecutive runs
         * (imdct_run_body<..., RV>); block order forward or — g_rv == 2 — reversed */
        static unsigned long long epoch = 1000;
        std::vector<unsigned long long> rv_state((size_t)ph.n_links_rv * AACG_RV_STATE_WORDS + 1, 0x5a5a5a5a5a5a5a5aull);
        std::vector<float> rv_data((size_t)ph.n_links_rv * AACG_RV_DATA_FLOATS + 1, std::numeric_limits<float>::quiet_NaN());
        std::vector<aacg_run> runs = ph.runs_rv;
        std::vector<aacg_rv_link> links = ph.links_rv;
        if (g_rv == 2) { std::reverse(runs.begin(), runs.end()); std::reverse(links.begin(), links.end()); }
        aacg_kparams K = P;
        K.runs = runs.data(); K.n_runs = (int32_t)runs.size(); K.scratch = nullptr;
        if (R.run_key & AACG_RK_EX) { K.pns = &pns_tab; if (ph.any_tns) aacg_set_tns_m(&K, tns_m.data()); }      /* optional stages inside the run kernel */
        aacg_rv_args V;
        std::memset(&V, 0, sizeof V);
        V.links = links.data(); V.state = rv_state.data(); V.data = rv_data.data(); V.epoch = ++epoch;
        if (g_cfg.policy == POL_CELL) {
            /* policy cell(a, variant): cell a of this launch, between the workgroup whose link_out it is and the one whose link_in */
            if (g_cfg.a < 0 || g_cfg.a >= (int)ph.n_links_rv) { g_err = "no such rendezvous cell"; return AACG_ERR_UNSUPPORTED; }
            g_watch.addr = rv_state.data() + (size_t)g_cfg.a * AACG_RV_STATE_WORDS;
            g_watch.variant = g_cfg.b;
            for (size_t b = 0; b < links.size(); b++) {
                if (links[b].link_out == g_cfg.a) g_watch.wg[0] = (int)b;
                if (links[b].link_in == g_cfg.a) g_watch.wg[1] = (int)b;
            }
        }
        launch(K, 1, R.run_key, (int)runs.size(), AACG_WG_WAVES, run_lds_bytes(R.run_key), 0, nullptr, nullptr, &V);
    } else {
        if (R.stage == AACG_STAGE_DEPENDENT_COUPLING) {
            spec.assign((size_t)ph.coef_blocks * 1024u, 0.0f);
            aacg_kparams Q = P;
            Q.spec_out = spec.data(); Q.pns = &pns_tab; Q.tns = nullptr;
            if (R.stage_quant) launch(Q, 3, 0, unit_blocks, AACG_WG_WAVES, (AACG_SPX_TAB_FLOATS + AACG_WG_WAVES * AACG_SPX_WAVE_FLOATS) * 4, (int)n_units);
            else std::memcpy(spec.data(), coeffs, spec.size() * sizeof(float));
            couple(AACG_CCE_BEFORE_TNS);
            if (ph.any_tns) {
                Q.coeffs = spec.data(); Q.meta = nullptr; Q.tns = ph.tns.data(); aacg_set_tns_m(&Q, tns_m.data());
                launch(Q, 4, 0, unit_blocks, AACG_WG_WAVES, AACG_WG_WAVES * AACG_SPX_WAVE_FLOATS * 4, (int)n_units);
            }
            couple(AACG_CCE_AFTER_TNS);
            P.coeffs = spec.data(); P.meta = nullptr; P.tns = nullptr;
        } else if (R.stage == AACG_STAGE_SPECTRAL_EX) {
            spec.assign((size_t)ph.coef_blocks * 1024u, 0.0f);
            aacg_kparams Q = P;
            Q.spec_out = spec.data(); Q.pns = &pns_tab; if (ph.any_tns) aacg_set_tns_m(&Q, tns_m.data());
            launch(Q, R.stage_quant ? 3 : 4, 0, unit_blocks, AACG_WG_WAVES, ((R.stage_quant ? AACG_SPX_TAB_FLOATS : 0) + AACG_WG_WAVES * AACG_SPX_WAVE_FLOATS) * 4, (int)n_units);
            P.coeffs = spec.data(); P.meta = nullptr; P.tns = nullptr;
        } else if (R.has_run && (R.run_key & AACG_RK_EX)) { P.pns = &pns_tab; if (ph.any_tns) aacg_set_tns_m(&P, tns_m.data()); }
        auto side_pass = [&]() {
            aacg_kparams C = P;
            C.runs = ph.cce_runs.data(); C.n_runs = (int32_t)ph.cce_runs.size(); C.pcm = side.data(); C.scratch = nullptr;
            launch(C, 1, R.side_key, (int)ph.cce_runs.size(), AACG_WG_WAVES, run_lds_bytes(R.side_key));
        };
        if (R.has_side && R.side_first) side_pass();
        if (R.has_run) {
            if (R.run_key & AACG_RK_CPL) aacg_set_cpl(&P, ph.couple_jobs.data() + ph.fused_first, ph.gains.data(), side.data());
            launch(P, 1, R.run_key, (int)ph.runs.size(), AACG_WG_WAVES, run_lds_bytes(R.run_key));
        }
        if (R.has_side && !R.side_first) side_pass();
        if (R.couple_pcm) couple(AACG_CCE_AFTER_IMDCT);
    }
    if (g_sched_failed) return EMU_ERR_DEADLOCK;
    for (auto& c : ph.chains)
        for (int k = 0; k < c.n_ch; k++) { uint8_t& b = parity[(size_t)c.stream * (size_t)max_channels + c.channel + k]; b = (uint8_t)((b + 1) % AACG_OV_BUFFERS); }
    return AACG_OK;
}

/* aacg_decode_pipelined (aacg_engine.hip) for n_launches consecutive launches of ONE plan: launch j reads the coefficient
 * blocks at coeffs[j] / meta[j] and writes pcm[j]; the chains of neighbouring launches meet in the cross-launch cells.  The
 * emulator runs one workgroup at a time, in an order the engine's ordering rules allow: only neighbouring launches overlap
 * (launch j + 2 starts after launch j is complete).  order: 0 = launch after launch; 1 = within every pair (j, j + 1) the LATER
 * launch's workgroups first (every consumer leaves its first half, every producer finishes a frame of the next launch);
 * >= 2: the workgroups of all launches the engine's ordering rules allow to be in flight, interleaved at random (seed = order).
 * xl_cells: [max_streams][max_channels][3] records of 4 x u64 (aacg_xl_cell), xl_head: like the overlap pool; both kept by the
 * caller so that a sequence can be continued by a later call (first_epoch_in: 0 = its input state is complete; else the epoch
 * the previous call returned in *last_epoch, i.e. that call's last launch is "still in flight"). */
int emu_decode_pipelined(int input_kind, int sample_index, int max_streams, int max_channels,
                         const aacg_unit_desc* units, uint32_t n_units, int n_launches, const void* const* coeffs, const aacg_band_meta* const* meta,
                         float* const* pcm, size_t n_pcm_floats, float* overlap_pool, uint8_t* parity,
                         void* xl_cells, float* xl_head, int order, unsigned long long first_epoch_in, unsigned long long* last_epoch, int streams)
{
    if (g_tab_index != sample_index) { int rc = aacg_build_tables(sample_index, &g_tab, nullptr); if (rc) return rc; g_tab_index = sample_index; }
    aacg_plan_host ph;
    int rc = aacg_plan_build(units, n_units, sample_index, max_streams, max_channels, parity, &ph, &g_err);
    if (rc) return rc;
    if (ph.pcm_floats > n_pcm_floats) { g_err = "pcm buffer too small"; return AACG_ERR_CAPACITY; }
    const aacg_route R = aacg_pick_route(input_kind, AACG_OUTPUT_F32, 0, false, ph, true);
    g_keys.clear();
    if (!R.overlappable) { g_err = "not a plain batch"; return AACG_ERR_UNSUPPORTED; }
    static unsigned long long epoch = 5000;
    const int NS = streams > 0 ? streams : aacg_pipeline_streams(ph, R.run_key);          /* streams the sequence takes in turn (0: the engine's choice) */
    const size_t cells = (size_t)ph.n_links_rv;
    std::vector<unsigned long long> rv_state(AACG_PIPE_STREAMS * cells * AACG_RV_STATE_WORDS + 1, 0x5a5a5a5a5a5a5a5aull);
    std::vector<float> rv_data(AACG_PIPE_STREAMS * cells * AACG_RV_DATA_FLOATS + 1, std::numeric_limits<float>::quiet_NaN());
    std::vector<aacg_kparams> P((size_t)n_launches);
    std::vector<aacg_rv_args> V((size_t)n_launches);
    for (int j = 0; j < n_launches; j++) {
        if (ph.zero_fill) std::memset(pcm[j], 0, n_pcm_floats * 4);
        std::memset(&P[(size_t)j], 0, sizeof(aacg_kparams));
        aacg_kparams& p = P[(size_t)j];
        p.units = ph.units.data(); p.runs = ph.runs_rv.data(); p.coeffs = coeffs[j]; p.meta = meta ? meta[j] : nullptr; p.pcm = pcm[j];
        p.overlap = overlap_pool; p.tab = &g_tab; p.flip = j % AACG_OV_BUFFERS; p.n_runs = (int32_t)ph.runs_rv.size();
        aacg_rv_args& v = V[(size_t)j];
        std::memset(&v, 0, sizeof v);
        v.links = ph.links_rv.data();
        const size_t set = (size_t)aacg_pipeline_order((uint64_t)j, NS).stream;      /* launches in flight together never share a set of in-launch cells */
        v.state = rv_state.data() + set * cells * AACG_RV_STATE_WORDS;
        v.data = rv_data.data() + set * cells * AACG_RV_DATA_FLOATS;
        v.epoch = ++epoch;
        v.xl_cells = (aacg_xl_cell*)xl_cells; v.xl_head = xl_head;
        v.epoch_in = j ? V[(size_t)j - 1].epoch : first_epoch_in;
    }
    const int B = (int)ph.runs_rv.size();
    g_steps = 0; g_trace.clear(); g_sched_failed = false; g_watch = watch_cfg();
    g_last_links = (int)ph.n_links_rv; g_last_chains = 0;
    for (auto& r : ph.runs_rv) g_last_chains += r.is_last ? 1 : 0;
    if (g_cfg.policy != POL_OFF) {
        /* schedule-controlled mode (`order` is not used): the workgroups of every launch the engine's ordering rules allow in
         * flight — the rules of order >= 2 below — are resident together under the one controller; a launch's workgroups join
         * when the launches it has to wait for are complete */
        for (int j = 0; j < n_launches; j++) g_keys.push_back(R.run_key);
        sched_state s;
        sched_init(s);
        if (g_cfg.policy == POL_CELL) {
            /* policy cell(a, variant): the cross-launch cell of chain a % chains between launches a / chains and a / chains + 1 */
            const int j = g_last_chains ? g_cfg.a / g_last_chains : -1, c = g_last_chains ? g_cfg.a % g_last_chains : 0;
            if (g_cfg.a < 0 || j + 1 >= n_launches) { g_err = "no such cross-launch cell"; return AACG_ERR_UNSUPPORTED; }
            int seen = 0;
            for (auto& r : ph.runs_rv) {
                if (!r.is_last || seen++ != c) continue;
                s.watch.addr = &((aacg_xl_cell*)xl_cells + ((r.ov0[0] >> 10) + ov_buffer(r.rot[0], P[(size_t)j].flip + 1)))->state;
            }
            s.watch.variant = g_cfg.b;
            s.watch.launch[0] = j; s.watch.launch[1] = j + 1;
        }
        std::vector<char> started((size_t)n_launches, 0);
        s.waves_left.assign((size_t)n_launches, 0);
        auto done = [&](int j) { return j < 0 || (started[(size_t)j] && s.waves_left[(size_t)j] == 0); };
        s.progress = [&]() {
            for (int j = 0; j < n_launches; j++) {
                if (started[(size_t)j] || !done(j - NS)) continue;
                const aacg_pipe_order o = aacg_pipeline_order((uint64_t)j, NS);
                bool known = true;
                for (int m = 0; m <= (int)o.complete_upto && known; m++) known = done(m);
                if (!known) continue;
                started[(size_t)j] = 1;
                for (int b = 0; b < B; b++) sched_add_wg(s, j, &P[(size_t)j], R.run_key, b, AACG_WG_WAVES, run_lds_bytes(R.run_key), &V[(size_t)j]);
            }
        };
        rc = sched_run(s);
        if (rc) return rc;
        for (auto& c : ph.chains)
            for (int k = 0; k < c.n_ch; k++) { uint8_t& b = parity[(size_t)c.stream * (size_t)max_channels + c.channel + k]; b = (uint8_t)((b + n_launches) % AACG_OV_BUFFERS); }
        if (last_epoch) *last_epoch = n_launches ? V[(size_t)n_launches - 1].epoch : first_epoch_in;
        return AACG_OK;
    }
    std::vector<std::pair<int, int>> sched;               /* (launch, block) */
    if (order == 0) {
        for (int j = 0; j < n_launches; j++) for (int b = 0; b < B; b++) sched.emplace_back(j, b);
    } else if (order == 1) {
        /* as late as the streams allow: of every NS consecutive launches the last one first */
        for (int j = 0; j < n_launches; j += NS)
            for (int k = NS - 1; k >= 0; k--)
                if (j + k < n_launches) for (int b = 0; b < B; b++) sched.emplace_back(j + k, b);
    } else {
        /* the engine's ordering rules, exactly (aacg_pipeline_order, aacg_routes.cpp): launch j goes to stream j mod
         * NS, so it starts after the launch NS before it is complete, and it does not exist before
         * the launches the host waits for are complete.  Among the launches those rules allow to run, the next workgroup is drawn at random, in each launch's
         * own shuffled block order */
        uint32_t rng = (uint32_t)order * 2654435761u + 12345u;
        auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 17; rng ^= rng << 5; return rng; };
        std::vector<std::vector<int>> left((size_t)n_launches);
        for (int j = 0; j < n_launches; j++) {
            for (int b = 0; b < B; b++) left[(size_t)j].push_back(b);
            for (int b = B - 1; b > 0; b--) std::swap(left[(size_t)j][(size_t)b], left[(size_t)j][next() % (uint32_t)(b + 1)]);
        }
        auto done = [&](int j) { return j < 0 || left[(size_t)j].empty(); };
        size_t remaining = (size_t)n_launches * (size_t)B;
        while (remaining) {
            std::vector<int> ready;
            for (int j = 0; j < n_launches; j++) {
                const aacg_pipe_order o = aacg_pipeline_order((uint64_t)j, NS);
                if (left[(size_t)j].empty() || !done(j - NS)) continue;
                bool known = true;                          /* the host enqueues it only after everything up to complete_upto is complete */
                for (int m = 0; m <= (int)o.complete_upto && known; m++) known = done(m);
                if (!known) continue;
                ready.push_back(j);
            }
            const int j = ready[next() % (uint32_t)ready.size()];
            sched.emplace_back(j, left[(size_t)j].back());
            left[(size_t)j].pop_back();
            remaining--;
        }
    }
    for (int j = 0; j < n_launches; j++) g_keys.push_back(R.run_key);
    for (auto& jb : sched)
        run_block(P[(size_t)jb.first], 1, R.run_key, jb.second, AACG_WG_WAVES, run_lds_bytes(R.run_key), 0, nullptr, nullptr, &V[(size_t)jb.first]);
    for (auto& c : ph.chains)
        for (int k = 0; k < c.n_ch; k++) { uint8_t& b = parity[(size_t)c.stream * (size_t)max_channels + c.channel + k]; b = (uint8_t)((b + n_launches) % AACG_OV_BUFFERS); }
    if (last_epoch) *last_epoch = n_launches ? V[(size_t)n_launches - 1].epoch : first_epoch_in;
    return AACG_OK;
}

int emu_spectral(int sample_index, const aacg_unit_desc* units, uint32_t n_units,
                 const void* coeffs, const aacg_band_meta* meta, float* spec_out)
{
    if (g_tab_index != sample_index) { int rc = aacg_build_tables(sample_index, &g_tab, nullptr); if (rc) return rc; g_tab_index = sample_index; }
    aacg_plan_host ph;
    int rc = aacg_plan_build(units, n_units, sample_index, 1 << 16, 8, nullptr, &ph, &g_err);
    if (rc) return rc;
    aacg_kparams P;
    std::memset(&P, 0, sizeof P);
    P.units = ph.units.data(); P.coeffs = coeffs; P.meta = meta; P.spec_out = spec_out; P.tab = &g_tab;
    launch(P, 2, 0, (int)((n_units + AACG_WG_WAVES - 1) / AACG_WG_WAVES), AACG_WG_WAVES,
           (AACG_TAB_QUANT_FLOATS + AACG_WG_WAVES * 512) * 4, (int)n_units);
    return AACG_OK;
}

/* the device front end (aacg_parse.h) on host memory: same arguments as aacg_parse_batch */
int emu_parse(int sample_index, const aacg_code_entry* entries, const uint32_t* counts,
              const uint8_t* bytes, size_t n_bytes, const aacg_parse_frame* frames, uint32_t n_frames,
              uint32_t max_units, uint32_t max_channels, uint32_t options,
              aacg_unit_desc* units, int16_t* q, aacg_band_meta* meta, aacg_tns_info* tns, aacg_parse_result* results)
{
    static aacg_parse_tables tab;
    int rc = aacg_parse_build_tables(sample_index, entries, counts, &tab, &g_err);
    if (rc) return rc;
    std::vector<uint32_t> padded((n_bytes + 15) / 16 * 4 + AACG_PARSE_PAD_BYTES / 4 + 4, 0u);
    std::memcpy(padded.data(), bytes, n_bytes);
    const size_t blocks = (size_t)n_frames * max_channels;
    std::memset(units, 0, (size_t)n_frames * max_units * sizeof *units);
    std::memset(q, 0, blocks * 1024 * sizeof *q);
    std::memset(meta, 0, blocks * sizeof *meta);
    if (tns) std::memset(tns, 0, blocks * sizeof *tns);
    aacg_parse_params PP;
    PP.bytes = padded.data(); PP.frames = frames; PP.tab = &tab; PP.units = units; PP.q = q; PP.meta = meta; PP.tns = tns; PP.results = results;
    PP.n_frames = n_frames; PP.max_units = max_units; PP.max_channels = max_channels; PP.options = options;
    /* AACG_EMU_ARENA: a small staging arena sends most frames down the read-in-place path */
    PP.wg_threads = AACG_PARSE_WG_SMALL;
    /* the launcher's lane order: frames sorted by length (a host sort here, a counting sort on the device), the sorted
     * 64-frame pieces dealt out to the workgroups in turn; idle lanes carry 0xffffffff */
    const uint32_t n_wg = (n_frames + PP.wg_threads - 1) / PP.wg_threads, waves = PP.wg_threads / 64;
    std::vector<uint32_t> sorted(n_frames), order((size_t)n_wg * PP.wg_threads, 0xffffffffu);
    for (uint32_t i = 0; i < n_frames; i++) sorted[i] = i;
    std::stable_sort(sorted.begin(), sorted.end(), [&](uint32_t a, uint32_t b) { return frames[a].byte_length > frames[b].byte_length; });
    for (uint32_t pos = 0; pos < n_frames; pos++) {
        const uint32_t piece = pos >> 6;
        order[((piece % n_wg) * waves + piece / n_wg) * 64u + (pos & 63u)] = sorted[pos];
    }
    PP.order = n_frames > 64 ? order.data() : nullptr;
    const size_t fixed = AACG_PARSE_LDS_FIXED(tab.lut_words, PP.wg_threads);
    const char* env = std::getenv("AACG_EMU_ARENA");
    PP.arena_bytes = env ? (uint32_t)std::atoi(env) : (uint32_t)(160 * 1024 - fixed);
    aacg_kparams none;
    std::memset(&none, 0, sizeof none);
    launch(none, 7, 0, (int)((n_frames + PP.wg_threads - 1) / PP.wg_threads), (int)PP.wg_threads / 64,
           fixed + PP.arena_bytes, 0, &PP);
    return AACG_OK;
}

}  // extern "C"
