// GPU test program (run by tests/test_gpu_group_rollout.py): disturbed closed-loop rollouts through the multi-GPU C ABI
// (ismpc_group_rollout_mc_device / ismpc_a_group_rollout_mc_device, include/ismpc_group.h) with 1 rank on the real RCCL and with 2, 3
// and 8 ranks on the one GPU of the test box through the in-process RCCL test double (tests/helpers/fake_rccl.cpp, selected with
// ISMPC_RCCL_LIB; this process maps no torch).  What exists only for world > 1 -- the summary written at summary_all + first, the
// trajectory block at traj_all + first * rows, the two in-place all-gathers of one fused group, the per-root broadcasts of ragged
// batches, ranks with an empty shard, the wait before the next rollout rewrites the caller's buffers -- is checked by bytes.
// Yardstick: a plain handle called once PER SHARD (ismpc_rollout_mc_device / ismpc_a_rollout_mc_device of the shard's count records;
// for Formulation A a fresh handle per shard), its tick-major trajectory transposed on the host.  Every comparison is memcmp, on
// EVERY local device: the whole summary_all and traj_all, the device's final shard states, and the bytes behind batch * rows records.
//   usage: test_group_rollout <world> <tick_in.bin> <a_state.bin> <a_inst.bin>
//   world 1: the bound RCCL must be a real one (version > 20000); world 2..8: the test double (version 1)
//   with ISMPC_GROUP_FORCE_RAGGED=1: the batches whose shards are equal (4096, 768) only, through the all-gather-v form
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

#include "ismpc_group.h"

#define CHECK(cond, ...) do { if (!(cond)) { std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); std::fprintf(stderr, __VA_ARGS__); \
    std::fprintf(stderr, " [group: %s] [ismpc: %s] [a: %s]\n", ismpc_group_last_error(), ismpc_last_error(), ismpc_a_last_error()); return 1; } } while (0)
#define HIP_OK(expr) CHECK((expr) == hipSuccess, #expr)

typedef unsigned char u8;
enum { B_MAX = 4099, A_MAX = 768, MAX_ROWS = 24, GUARD = 64, REC = 80, FILL = 0xEE, MAX_PUSH = 2 };

template <typename T> static bool read_file(const char* path, std::vector<T>& v, size_t n)
{
    v.resize(n);
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    const size_t got = std::fread(v.data(), sizeof(T), n, f);
    std::fclose(f);
    return got == n;
}

// first record of `bytes` bytes that differs, or -1
static long first_diff(const u8* a, const u8* b, size_t n, size_t bytes)
{
    for (size_t i = 0; i < n; ++i) if (std::memcmp(a + i * bytes, b + i * bytes, bytes) != 0) return (long)i;
    return -1;
}
static long first_not_fill(const u8* a, size_t from, size_t to)
{
    for (size_t i = from; i < to; ++i) if (a[i] != FILL) return (long)i;
    return -1;
}

// One formulation as the harness sees it: record sizes, and the plain and the group call over untyped pointers.
struct Rig {
    int world = 0, max_batch = 0;
    size_t state_b = 0, inst_b = 0, push_b = 0, sum_b = 0;
    std::function<int(int count, void* st, const void* inst, const void* push, int n_push, int ticks, int stride, void* traj, void* sum)> plain;
    std::function<int(int batch, void* const* st, const void* const* inst, const void* const* push, int n_push, int ticks, int stride, void* const* traj, void* const* sum)> group;
    std::function<int(int l, void* stream)> wait_on, order_after;
    std::function<int()> sync;
    // per local device: two sets of shard inputs (set 1: what a second call reads while the first still runs), the caller's gathered buffers
    u8 *d_st[2][8] = {}, *d_push[2][8] = {}, *d_inst[8] = {}, *d_traj[8] = {}, *d_sum[8] = {};
    u8 *y_st = nullptr, *y_inst = nullptr, *y_push = nullptr, *y_traj = nullptr, *y_sum = nullptr;      // the yardstick's
    size_t traj_cap() const { return ((size_t)max_batch * MAX_ROWS + GUARD) * REC; }
    size_t sum_cap() const { return ((size_t)max_batch + GUARD) * sum_b; }
};
struct Ref { int rows = 0; std::vector<u8> state, traj, sum; };   // traj instance-major

static int rig_alloc(Rig& r)
{
    const size_t n = (size_t)r.max_batch;
    for (int l = 0; l < r.world; ++l) {
        for (int s = 0; s < 2; ++s) { HIP_OK(hipMalloc((void**)&r.d_st[s][l], n * r.state_b)); HIP_OK(hipMalloc((void**)&r.d_push[s][l], n * MAX_PUSH * r.push_b)); }
        HIP_OK(hipMalloc((void**)&r.d_inst[l], n * (r.inst_b ? r.inst_b : 1)));
        HIP_OK(hipMalloc((void**)&r.d_traj[l], r.traj_cap())); HIP_OK(hipMalloc((void**)&r.d_sum[l], r.sum_cap()));
    }
    HIP_OK(hipMalloc((void**)&r.y_st, n * r.state_b)); HIP_OK(hipMalloc((void**)&r.y_push, n * MAX_PUSH * r.push_b));
    HIP_OK(hipMalloc((void**)&r.y_inst, n * (r.inst_b ? r.inst_b : 1)));
    HIP_OK(hipMalloc((void**)&r.y_traj, n * MAX_ROWS * REC)); HIP_OK(hipMalloc((void**)&r.y_sum, n * r.sum_b));
    return 0;
}
static void rig_free(Rig& r)
{
    for (int l = 0; l < r.world; ++l) {
        for (int s = 0; s < 2; ++s) { (void)hipFree(r.d_st[s][l]); (void)hipFree(r.d_push[s][l]); }
        (void)hipFree(r.d_inst[l]); (void)hipFree(r.d_traj[l]); (void)hipFree(r.d_sum[l]);
    }
    (void)hipFree(r.y_st); (void)hipFree(r.y_push); (void)hipFree(r.y_inst); (void)hipFree(r.y_traj); (void)hipFree(r.y_sum);
}

// the yardstick: the plain call shard by shard, the trajectory transposed on the host
static int yard(Rig& r, int batch, const u8* states, const u8* inst, const u8* pushes, int n_push, int ticks, int stride, Ref& ref)
{
    const int rows = ticks / stride;
    ref.rows = rows;
    ref.state.assign((size_t)batch * r.state_b, 0); ref.traj.assign((size_t)batch * rows * REC, 0); ref.sum.assign((size_t)batch * r.sum_b, 0);
    std::vector<u8> tmp;
    int covered = 0;
    for (int k = 0; k < r.world; ++k) {
        int first, count;
        CHECK(ismpc_shard_range(batch, k, r.world, &first, &count) == ISMPC_OK && first == covered, "shard %d", k);
        covered += count;
        if (count == 0) continue;
        HIP_OK(hipMemcpy(r.y_st, states + (size_t)first * r.state_b, (size_t)count * r.state_b, hipMemcpyHostToDevice));
        if (inst) HIP_OK(hipMemcpy(r.y_inst, inst + (size_t)first * r.inst_b, (size_t)count * r.inst_b, hipMemcpyHostToDevice));
        if (n_push) HIP_OK(hipMemcpy(r.y_push, pushes + (size_t)first * n_push * r.push_b, (size_t)count * n_push * r.push_b, hipMemcpyHostToDevice));
        CHECK(r.plain(count, r.y_st, inst ? r.y_inst : nullptr, n_push ? r.y_push : nullptr, n_push, ticks, stride, r.y_traj, r.y_sum) == ISMPC_OK, "yardstick shard %d", k);
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(&ref.state[(size_t)first * r.state_b], r.y_st, (size_t)count * r.state_b, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(&ref.sum[(size_t)first * r.sum_b], r.y_sum, (size_t)count * r.sum_b, hipMemcpyDeviceToHost));
        tmp.resize((size_t)rows * count * REC + 1);
        if (rows) HIP_OK(hipMemcpy(tmp.data(), r.y_traj, (size_t)rows * count * REC, hipMemcpyDeviceToHost));
        for (int t = 0; t < rows; ++t) for (int i = 0; i < count; ++i)
            std::memcpy(&ref.traj[((size_t)(first + i) * rows + t) * REC], &tmp[((size_t)t * count + i) * REC], REC);
    }
    CHECK(covered == batch, "shards cover %d of %d", covered, batch);
    return 0;
}

// the shards' inputs to set `set` of every local device
static int upload(Rig& r, int set, int batch, const u8* states, const u8* inst, const u8* pushes, int n_push)
{
    for (int l = 0; l < r.world; ++l) {
        int first, count; ismpc_shard_range(batch, l, r.world, &first, &count);
        if (count == 0) continue;
        HIP_OK(hipMemcpy(r.d_st[set][l], states + (size_t)first * r.state_b, (size_t)count * r.state_b, hipMemcpyHostToDevice));
        if (inst) HIP_OK(hipMemcpy(r.d_inst[l], inst + (size_t)first * r.inst_b, (size_t)count * r.inst_b, hipMemcpyHostToDevice));
        if (n_push) HIP_OK(hipMemcpy(r.d_push[set][l], pushes + (size_t)first * n_push * r.push_b, (size_t)count * n_push * r.push_b, hipMemcpyHostToDevice));
    }
    return 0;
}
// the caller's output buffers, whole, to the fill byte; the group's launch streams are ordered behind it
static int fill(Rig& r)
{
    for (int l = 0; l < r.world; ++l) {
        HIP_OK(hipMemsetAsync(r.d_traj[l], FILL, r.traj_cap(), nullptr)); HIP_OK(hipMemsetAsync(r.d_sum[l], FILL, r.sum_cap(), nullptr));
        CHECK(r.order_after(l, nullptr) == ISMPC_OK, "order_after");
    }
    return 0;
}
// the group call: empty shards pass NULL
static int launch(Rig& r, int set, int batch, bool with_inst, int n_push, int ticks, int stride, bool want_traj, bool want_sum)
{
    void* st[8] = {}; const void* in[8] = {}; const void* pu[8] = {};
    for (int l = 0; l < r.world; ++l) {
        int first, count; ismpc_shard_range(batch, l, r.world, &first, &count);
        if (count == 0) continue;
        st[l] = r.d_st[set][l]; in[l] = with_inst ? r.d_inst[l] : nullptr; pu[l] = n_push ? r.d_push[set][l] : nullptr;
    }
    return r.group(batch, st, with_inst ? in : nullptr, n_push ? pu : nullptr, n_push, ticks, stride, want_traj ? (void* const*)r.d_traj : nullptr, want_sum ? (void* const*)r.d_sum : nullptr);
}
// every local device, on a caller stream behind rollout_wait_on: the gathered buffers, what lies behind them, the shard's final states
static int check(Rig& r, int set, int batch, const Ref& ref, bool want_traj, bool want_sum, const char* what)
{
    std::vector<u8> traj(r.traj_cap()), sum(r.sum_cap()), st((size_t)r.max_batch * r.state_b);
    hipStream_t s; HIP_OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    for (int l = 0; l < r.world; ++l) {
        int first, count; ismpc_shard_range(batch, l, r.world, &first, &count);
        CHECK(r.wait_on(l, s) == ISMPC_OK, "rollout_wait_on");
        HIP_OK(hipMemcpyAsync(traj.data(), r.d_traj[l], traj.size(), hipMemcpyDeviceToHost, s));
        HIP_OK(hipMemcpyAsync(sum.data(), r.d_sum[l], sum.size(), hipMemcpyDeviceToHost, s));
        if (count) HIP_OK(hipMemcpyAsync(st.data(), r.d_st[set][l], (size_t)count * r.state_b, hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
        const size_t tb = want_traj ? (size_t)batch * ref.rows * REC : 0, sb = want_sum ? (size_t)batch * r.sum_b : 0;
        long d = want_traj ? first_diff(traj.data(), ref.traj.data(), (size_t)batch * ref.rows, REC) : -1;
        CHECK(d < 0, "%s, local device %d: trajectory record %ld (instance %ld, row %ld) differs from the per-shard yardstick", what, l, d, d / (ref.rows ? ref.rows : 1), d % (ref.rows ? ref.rows : 1));
        d = first_not_fill(traj.data(), tb, traj.size());
        CHECK(d < 0, "%s, local device %d: trajectory byte %ld outside the %zu bytes of the result was written", what, l, d, tb);
        d = want_sum ? first_diff(sum.data(), ref.sum.data(), (size_t)batch, r.sum_b) : -1;
        CHECK(d < 0, "%s, local device %d: summary %ld differs from the per-shard yardstick", what, l, d);
        d = first_not_fill(sum.data(), sb, sum.size());
        CHECK(d < 0, "%s, local device %d: summary byte %ld outside the %zu bytes of the result was written", what, l, d, sb);
        d = first_diff(st.data(), &ref.state[(size_t)first * r.state_b], (size_t)count, r.state_b);
        CHECK(d < 0, "%s, local device %d: final state %ld of the shard differs from the per-shard yardstick", what, l, d);
    }
    HIP_OK(hipStreamDestroy(s));
    return 0;
}

// Push tables, instance-major, two entries per instance; variant 0 / 1 differ in ticks and signs.  A third of the instances (all of a
// tiny batch, so that every shard holds one) is shoved hard at an early tick: `hard` m/s on x and -y.
template <typename P> static void make_pushes(std::vector<P>& t, int batch, int variant, double hard, int dims)
{
    t.assign((size_t)batch * 2, P());
    for (int i = 0; i < batch; ++i) {
        P& a = t[2 * (size_t)i]; P& b = t[2 * (size_t)i + 1];
        const bool shove = i % 3 == 0 || batch <= 8;
        const double sg = variant ? -1.0 : 1.0;
        a.tick = (i + variant) % 3; a.reserved = 0;
        a.dv[0] = sg * (shove ? hard : 0.004 * (i % 5)); a.dv[1] = -sg * (shove ? hard : 0.003 * (i % 7));
        b.tick = i % 11 == 10 ? INT_MAX : 5 + (i + 2 * variant) % 4; b.reserved = 0;
        b.dv[0] = -sg * 0.002 * (i % 9); b.dv[1] = sg * 0.005 * (i % 4);
        if (dims > 2) { a.dv[2] = 0.0; b.dv[2] = sg * 0.001 * (i % 3); }
    }
}

struct Case { int ticks, stride; };

// the cases of one formulation: batches x (ticks, stride) x pushes x outputs; returns the number of group calls checked, or -1
template <typename P, typename ErrTick>
static int run_cases(Rig& r, const char* name, const int* batches, int n_batches, const Case* cases, int n_cases, const u8* states, const u8* inst,
                     double hard, int dims, ErrTick first_error_tick)
{
    int done = 0;
    char what[160];
    for (int bi = 0; bi < n_batches; ++bi) for (int ci = 0; ci < n_cases; ++ci) for (int n_push = 0; n_push <= 2; n_push += 2) {
        const int batch = batches[bi], ticks = cases[ci].ticks, stride = cases[ci].stride;
        std::vector<P> pushes; make_pushes(pushes, batch, 0, hard, dims);
        Ref ref;
        if (yard(r, batch, states, inst, (const u8*)pushes.data(), n_push, ticks, stride, ref)) return -1;
        if (n_push && ticks >= 12) for (int k = 0; k < r.world; ++k) {          // a condition on the inputs: every shard holds an instance the shove broke
            int first, count, broken = 0; ismpc_shard_range(batch, k, r.world, &first, &count);
            for (int i = first; i < first + count; ++i) broken += first_error_tick(&ref.sum[(size_t)i * r.sum_b]) >= 0;
            if (count && !broken) { std::fprintf(stderr, "FAIL %s batch %d: no instance of shard %d carries an error bit in its summary\n", name, batch, k); return -1; }
        }
        for (int outs = 0; outs < 3; ++outs) {                                   // both, summary only, trajectory only
            const bool want_traj = outs != 1, want_sum = outs != 2;
            std::snprintf(what, sizeof what, "%s batch %d ticks %d stride %d n_push %d traj %d summary %d", name, batch, ticks, stride, n_push, (int)want_traj, (int)want_sum);
            if (upload(r, 0, batch, states, inst, (const u8*)pushes.data(), n_push) || fill(r)) return -1;
            if (launch(r, 0, batch, inst != nullptr, n_push, ticks, stride, want_traj, want_sum) != ISMPC_OK) { std::fprintf(stderr, "FAIL %s: the group call: %s\n", what, ismpc_group_last_error()); return -1; }
            if (check(r, 0, batch, ref, want_traj, want_sum, what)) return -1;
            ++done;
        }
    }
    return done;
}

int main(int argc, char** argv)
{
    if (argc < 5) { std::fprintf(stderr, "usage: test_group_rollout <world> <tick_in.bin> <a_state.bin> <a_inst.bin>\n"); return 2; }
    const int world = std::atoi(argv[1]);
    const bool ragged = std::getenv("ISMPC_GROUP_FORCE_RAGGED") != nullptr;
    CHECK(world >= 1 && world <= 8, "world %d", world);
    const int version = ismpc_group_rccl_version();
    if (world == 1) CHECK(version > 20000, "world 1 runs on the real RCCL: bound version %d", version);
    else CHECK(version == 1, "the test double is not the bound RCCL: version %d", version);
    std::vector<int> devices((size_t)world, 0);
    int b_calls = 0, a_calls = 0;

    // ================================================== Formulation B ==================================================
    {
        std::vector<ismpc_tick_in> in;
        CHECK(read_file(argv[2], in, (size_t)B_MAX), "reading %s", argv[2]);
        ismpc_params p; ismpc_params_default(&p);
        CHECK(p.N == 100, "N %d", p.N);
        const int rows = 40;
        std::vector<double> ftsp((size_t)rows * 4, 0.0);
        for (int i = 1; i < rows; ++i) {
            ftsp[4 * i + 0] = (i - 1) * 0.2; ftsp[4 * i + 1] = ((i - 1) % 2 == 0 ? 1.0 : -1.0) * 0.08;
            ftsp[4 * i + 3] = (p.mpc_dt / p.control_dt) * (p.S + p.F) * i;
        }
        ismpc_handle* h = nullptr; ismpc_group* g = nullptr;
        CHECK(ismpc_create(&p, ftsp.data(), rows, 0, &h) == ISMPC_OK, "ismpc_create");
        CHECK(ismpc_group_create(&p, ftsp.data(), rows, devices.data(), world, &g) == ISMPC_OK, "ismpc_group_create on %d x device 0", world);
        CHECK(ismpc_group_world(g) == world && ismpc_group_local(g) == world, "world %d local %d", ismpc_group_world(g), ismpc_group_local(g));
        CHECK(ismpc_group_rollout_wait_on(g, 0, nullptr) == ISMPC_OK, "rollout_wait_on before the first rollout is a no-op");

        int first_frame = 0;
        Rig r; r.world = world; r.max_batch = B_MAX;
        r.state_b = sizeof(ismpc_tick_in); r.push_b = sizeof(ismpc_push); r.sum_b = sizeof(ismpc_rollout_summary);
        r.plain = [&](int count, void* st, const void*, const void* push, int n_push, int ticks, int stride, void* traj, void* sum) {
            return ismpc_rollout_mc_device(h, count, (ismpc_tick_in*)st, first_frame, ticks, (const ismpc_push*)push, n_push, stride, (ismpc_tick_out*)traj, (ismpc_rollout_summary*)sum, nullptr); };
        r.group = [&](int batch, void* const* st, const void* const*, const void* const* push, int n_push, int ticks, int stride, void* const* traj, void* const* sum) {
            return ismpc_group_rollout_mc_device(g, batch, (ismpc_tick_in* const*)st, first_frame, ticks, (const ismpc_push* const*)push, n_push, stride,
                                                 (ismpc_tick_out* const*)traj, (ismpc_rollout_summary* const*)sum); };
        r.wait_on = [&](int l, void* s) { return ismpc_group_rollout_wait_on(g, l, s); };
        r.order_after = [&](int l, void* s) { return ismpc_group_order_after(g, l, s); };
        r.sync = [&]() { return ismpc_group_sync(g); };
        if (rig_alloc(r)) return 1;
        const u8* states = (const u8*)in.data();
        auto err_tick = [](const u8* s) { return ((const ismpc_rollout_summary*)s)->first_error_tick; };

        // ---- degenerate shapes and argument errors (nothing is enqueued by the refused calls)
        {
            void* st[8]; for (int l = 0; l < world; ++l) st[l] = r.d_st[0][l];
            CHECK(ismpc_group_rollout_mc_device(g, 0, nullptr, 0, 24, nullptr, 0, 1, nullptr, nullptr) == ISMPC_OK, "batch 0");
            CHECK(ismpc_group_rollout_mc_device(g, 64, nullptr, 0, 24, nullptr, 0, 1, nullptr, nullptr) == ISMPC_E_INVALID, "null state list");
            CHECK(ismpc_group_rollout_mc_device(g, 64, (ismpc_tick_in* const*)st, 0, 24, nullptr, 0, 0, nullptr, nullptr) == ISMPC_E_INVALID, "stride 0");
            CHECK(ismpc_group_rollout_mc_device(g, 64, (ismpc_tick_in* const*)st, -1, 24, nullptr, 0, 1, nullptr, nullptr) == ISMPC_E_INVALID, "negative first_frame");
            CHECK(ismpc_group_rollout_mc_device(g, 64, (ismpc_tick_in* const*)st, 0, 24, nullptr, 2, 1, nullptr, nullptr) == ISMPC_E_INVALID, "n_push 2 without tables");
            void* bad[8]; for (int l = 0; l < world; ++l) bad[l] = r.d_traj[l]; bad[world - 1] = nullptr;
            CHECK(ismpc_group_rollout_mc_device(g, 64, (ismpc_tick_in* const*)st, 0, 24, nullptr, 0, 1, (ismpc_tick_out* const*)bad, nullptr) == ISMPC_E_INVALID, "null trajectory entry");
            CHECK(ismpc_group_rollout_mc_device(g, 64, (ismpc_tick_in* const*)st, 0, 24, nullptr, 0, 1, nullptr, (ismpc_rollout_summary* const*)bad) == ISMPC_E_INVALID, "null summary entry");
            bad[world - 1] = r.d_traj[world - 1] + 8;
            CHECK(ismpc_group_rollout_mc_device(g, 64, (ismpc_tick_in* const*)st, 0, 24, nullptr, 0, 1, (ismpc_tick_out* const*)bad, nullptr) == ISMPC_E_INVALID, "misaligned trajectory");
            CHECK(std::strstr(ismpc_group_last_error(), "aligned") != nullptr, "last error: %s", ismpc_group_last_error());
            st[0] = nullptr;
            CHECK(ismpc_group_rollout_mc_device(g, 64, (ismpc_tick_in* const*)st, 0, 24, nullptr, 0, 1, nullptr, nullptr) == ISMPC_E_INVALID, "null state shard");
        }

        // ---- the cases: rows 24, 4 (with unrecorded tail ticks), 0 (ticks < stride), and ticks = 0
        const int batches[3] = {4096, 4099, 5};
        const Case cases[4] = {{24, 1}, {24, 5}, {3, 5}, {0, 1}};
        b_calls = run_cases<ismpc_push>(r, "B", batches, ragged ? 1 : 3, cases, 4, states, nullptr, 1.0, 3, err_tick);
        if (b_calls < 0) return 1;
        {   // ticks = 0: the empty summary of ismpc.h (the cases above found the group's bytes equal to these on every device; here, what they are)
            Ref z;
            if (yard(r, 5, states, nullptr, nullptr, 0, 0, 1, z)) return 1;
            ismpc_rollout_summary e; std::memcpy(&e, &z.sum[4 * sizeof e], sizeof e);
            CHECK(e.status_or == 0 && e.first_error_tick == -1 && e.error_ticks == 0 && e.fallback_ticks == 0 && e.com_z_min > 1e300 && e.com_z_max < -1e300
                  && e.max_abs_vel[0] == 0.0 && e.max_abs_vel[1] == 0.0, "the empty summary");
        }

        if (!ragged) {
            // ---- sequencing, no synchronisation in between: rollout (table 0) -> one tick step -> rollout (table 1) into the SAME output buffers
            const int batch = B_MAX, ticks = 24;
            std::vector<ismpc_push> t0, t1; make_pushes(t0, batch, 0, 1.0, 3); make_pushes(t1, batch, 1, 1.0, 3);
            Ref ref0, ref1;
            if (yard(r, batch, states, nullptr, (const u8*)t0.data(), 2, ticks, 1, ref0) || yard(r, batch, states, nullptr, (const u8*)t1.data(), 2, ticks, 1, ref1)) return 1;
            CHECK(first_diff(ref0.sum.data(), ref1.sum.data(), (size_t)batch, r.sum_b) >= 0 && std::memcmp(ref0.traj.data(), ref1.traj.data(), ref0.traj.size()) != 0,
                  "the two push tables give the same results: a stale buffer could not be seen");
            std::vector<ismpc_tick_out> tick_ref((size_t)batch), tick_got((size_t)batch);
            ismpc_tick_in* d_tin = nullptr; ismpc_tick_out* d_tout = nullptr;
            HIP_OK(hipMalloc((void**)&d_tin, sizeof(ismpc_tick_in) * (size_t)batch)); HIP_OK(hipMalloc((void**)&d_tout, sizeof(ismpc_tick_out) * (size_t)batch));
            HIP_OK(hipMemcpy(d_tin, in.data(), sizeof(ismpc_tick_in) * (size_t)batch, hipMemcpyHostToDevice));
            const ismpc_tick_in* tick_shards[8] = {};
            for (int k = 0; k < world; ++k) {
                int first, count; ismpc_shard_range(batch, k, world, &first, &count);
                tick_shards[k] = d_tin + first;
                CHECK(ismpc_solve_batch_device(h, count, d_tin + first, d_tout, nullptr, nullptr) == ISMPC_OK, "tick yardstick");
                HIP_OK(hipDeviceSynchronize());
                HIP_OK(hipMemcpy(&tick_ref[first], d_tout, sizeof(ismpc_tick_out) * (size_t)count, hipMemcpyDeviceToHost));
            }
            CHECK(ismpc_group_reserve(g, batch) == ISMPC_OK && ismpc_group_reserve_rollout(g, batch, ticks) == ISMPC_OK, "reserve");
            if (upload(r, 0, batch, states, nullptr, (const u8*)t0.data(), 2) || upload(r, 1, batch, states, nullptr, (const u8*)t1.data(), 2) || fill(r)) return 1;
            CHECK(launch(r, 0, batch, false, 2, ticks, 1, true, true) == ISMPC_OK, "first rollout");
            CHECK(ismpc_group_step_device(g, batch, tick_shards, 0) == ISMPC_OK, "the tick between the rollouts");
            CHECK(launch(r, 1, batch, false, 2, ticks, 1, true, true) == ISMPC_OK, "second rollout");
            if (check(r, 1, batch, ref1, true, true, "B second of two rollouts into the same buffers")) return 1;
            hipStream_t s; HIP_OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
            for (int l = 0; l < world; ++l) {
                int first, count; ismpc_shard_range(batch, l, world, &first, &count);
                ismpc_tick_out* res = nullptr;
                CHECK(ismpc_group_result_device(g, l, 0, &res) == ISMPC_OK && res, "result_device");
                CHECK(ismpc_group_wait_on(g, l, 0, s) == ISMPC_OK, "wait_on");
                HIP_OK(hipMemcpyAsync(tick_got.data(), res, sizeof(ismpc_tick_out) * (size_t)batch, hipMemcpyDeviceToHost, s));
                HIP_OK(hipStreamSynchronize(s));
                const long d = first_diff((const u8*)tick_got.data(), (const u8*)tick_ref.data(), (size_t)batch, sizeof(ismpc_tick_out));
                CHECK(d < 0, "the tick between two rollouts, local device %d: record %ld differs", l, d);
                std::vector<u8> st((size_t)count * r.state_b);      // the first rollout ran to its end too
                HIP_OK(hipMemcpy(st.data(), r.d_st[0][l], st.size(), hipMemcpyDeviceToHost));
                CHECK(first_diff(st.data(), &ref0.state[(size_t)first * r.state_b], (size_t)count, r.state_b) < 0, "first rollout's final states, local device %d", l);
            }
            HIP_OK(hipStreamDestroy(s));
            HIP_OK(hipFree(d_tin)); HIP_OK(hipFree(d_tout));
            b_calls += 2;

            // ---- a second call at first_frame + ticks continues the first (the states stay on their devices in between)
            Ref cont;
            first_frame = ticks;
            if (yard(r, batch, ref0.state.data(), nullptr, (const u8*)t0.data(), 2, ticks, 1, cont)) return 1;      // (a table's ticks count from 0 at each call)
            CHECK(first_diff(cont.sum.data(), ref0.sum.data(), (size_t)batch, r.sum_b) >= 0, "the continuation repeats the first call");
            first_frame = 0;
            if (upload(r, 0, batch, states, nullptr, (const u8*)t0.data(), 2) || fill(r)) return 1;
            CHECK(launch(r, 0, batch, false, 2, ticks, 1, true, true) == ISMPC_OK, "first of two consecutive rollouts");
            first_frame = ticks;
            CHECK(launch(r, 0, batch, false, 2, ticks, 1, true, true) == ISMPC_OK, "second of two consecutive rollouts");
            if (check(r, 0, batch, cont, true, true, "B rollout continued at first_frame + ticks")) return 1;
            first_frame = 0;
            b_calls += 2;
        }
        CHECK(ismpc_group_sync(g) == ISMPC_OK, "sync");
        rig_free(r);
        ismpc_group_destroy(g); ismpc_destroy(h);
    }

    // ================================================== Formulation A ==================================================
    {
        std::vector<ismpc_a_state> st0; std::vector<ismpc_a_inst> inst;
        CHECK(read_file(argv[3], st0, (size_t)A_MAX) && read_file(argv[4], inst, (size_t)A_MAX), "reading the A inputs");
        ismpc_a_params ap; ismpc_a_params_default(1, &ap);
        CHECK(ap.C == 100, "C %d", ap.C);
        ismpc_a_gait gait[2]; ismpc_a_gait_default(1, 0.78539816339744828, 0.1, &gait[0]); ismpc_a_gait_default(1, 0.78539816339744828, 0.12, &gait[1]);
        std::vector<double> fp((size_t)(gait[0].n_gait + 1) * 8), ce[2];
        for (int k = 0; k < 2; ++k) { ce[k].resize((size_t)gait[k].n_gait * 2); CHECK(ismpc_a_plan(&gait[k], fp.data(), ce[k].data()) > 0, "ismpc_a_plan"); }
        ismpc_a_group* ga = nullptr;
        CHECK(ismpc_a_group_create(&ap, ce[0].data(), devices.data(), world, &ga) == ISMPC_OK, "ismpc_a_group_create on %d x device 0", world);
        CHECK(ismpc_a_group_rollout_wait_on(ga, world - 1, nullptr) == ISMPC_OK, "rollout_wait_on before the first rollout is a no-op");
        bool second_plan = false, fp32 = false;
        Rig r; r.world = world; r.max_batch = A_MAX;
        r.state_b = sizeof(ismpc_a_state); r.inst_b = sizeof(ismpc_a_inst); r.push_b = sizeof(ismpc_a_push); r.sum_b = sizeof(ismpc_a_rollout_summary);
        r.plain = [&](int count, void* st, const void* in, const void* push, int n_push, int ticks, int stride, void* traj, void* sum) {
            ismpc_a_handle* ha = nullptr;                       // a fresh plain handle per shard, built the way the group's are
            if (ismpc_a_create(&ap, ce[0].data(), 0, &ha) != ISMPC_OK) return (int)ISMPC_E_INVALID;
            int rc = second_plan ? (ismpc_a_add_plan(ha, ce[1].data()) == 1 ? ISMPC_OK : ISMPC_E_INVALID) : ISMPC_OK;
            if (rc == ISMPC_OK && fp32) rc = ismpc_a_set_precision(ha, 1);
            if (rc == ISMPC_OK) rc = ismpc_a_rollout_mc_device(ha, count, (ismpc_a_state*)st, (const ismpc_a_inst*)in, ticks, (const ismpc_a_push*)push, n_push, stride,
                                                                (ismpc_a_out*)traj, (ismpc_a_rollout_summary*)sum, nullptr);
            if (hipDeviceSynchronize() != hipSuccess) rc = ISMPC_E_INVALID;
            ismpc_a_destroy(ha);
            return rc; };
        r.group = [&](int batch, void* const* st, const void* const* in, const void* const* push, int n_push, int ticks, int stride, void* const* traj, void* const* sum) {
            return ismpc_a_group_rollout_mc_device(ga, batch, (ismpc_a_state* const*)st, (const ismpc_a_inst* const*)in, ticks, (const ismpc_a_push* const*)push, n_push, stride,
                                                   (ismpc_a_out* const*)traj, (ismpc_a_rollout_summary* const*)sum); };
        r.wait_on = [&](int l, void* s) { return ismpc_a_group_rollout_wait_on(ga, l, s); };
        r.order_after = [&](int l, void* s) { return ismpc_a_group_order_after(ga, l, s); };
        r.sync = [&]() { return ismpc_a_group_sync(ga); };
        if (rig_alloc(r)) return 1;
        auto err_tick = [](const u8* s) { return ((const ismpc_a_rollout_summary*)s)->first_error_tick; };
        const int batches[2] = {768, 5};
        const Case cases[3] = {{12, 1}, {12, 4}, {0, 1}};
        CHECK(ismpc_a_group_reserve_rollout(ga, A_MAX, 12) == ISMPC_OK, "reserve_rollout");
        // the handles' parameters, fp64
        int n = run_cases<ismpc_a_push>(r, "A fp64", batches, ragged ? 1 : 2, cases, 3, (const u8*)st0.data(), nullptr, 2.0, 2, err_tick);
        if (n < 0) return 1;
        a_calls += n;
        // per-instance records over two plans, solved in fp32
        CHECK(ismpc_a_group_add_plan(ga, ce[1].data()) == 1 && ismpc_a_group_set_precision(ga, 1) == ISMPC_OK, "add_plan / set_precision");
        second_plan = true; fp32 = true;
        n = run_cases<ismpc_a_push>(r, "A inst fp32", batches, ragged ? 1 : 2, cases, 3, (const u8*)st0.data(), (const u8*)inst.data(), 2.0, 2, err_tick);
        if (n < 0) return 1;
        a_calls += n;
        CHECK(ismpc_a_group_sync(ga) == ISMPC_OK, "sync");
        rig_free(r);
        ismpc_a_group_destroy(ga);
    }
    std::printf("OK world=%d rccl=%d ragged=%s b_calls=%d a_calls=%d\n", world, version, ragged ? "forced" : "no", b_calls, a_calls);
    return 0;
}
