// GPU test program (run by tests/test_gpu_group.py): the multi-GPU C ABI (include/ismpc_group.h) with MORE THAN ONE RANK on the one
// GPU of the test box.  RCCL is the in-process test double tests/helpers/fake_rccl.cpp (selected with ISMPC_RCCL_LIB; this process
// maps no torch, so nothing else is bound), the group is built on devices {0, ..., 0}, and everything that exists only for
// world > 1 -- the offset rec * first of a shard in the gathered buffer, the in-place all-gather, the per-root broadcasts of ragged
// batches, ranks with an empty shard, the gathered[b] wait before a kernel rewrites buffer b, the host copies at in_host + first
// and the Formulation A state written back at state_host + first -- is checked by bytes.
// Yardstick: a plain handle called once PER SHARD (count records starting at first), which is what the header promises equality
// with; another batch size may select another lane layout.  Every comparison is memcmp.
//   usage: test_group_world <world> <tick_in.bin> <a_state.bin> <a_push.bin> <a_inst.bin>
//   with ISMPC_GROUP_FORCE_RAGGED=1: Formulation B at batch 4096 only, through the all-gather-v form (world roots at non-zero offsets)
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ismpc_group.h"

#define CHECK(cond, ...) do { if (!(cond)) { std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); std::fprintf(stderr, __VA_ARGS__); \
    std::fprintf(stderr, " [group: %s] [ismpc: %s] [a: %s]\n", ismpc_group_last_error(), ismpc_last_error(), ismpc_a_last_error()); return 1; } } while (0)
#define HIP_OK(expr) CHECK((expr) == hipSuccess, #expr)

enum { B_MAX = 4099, A_MAX = 768, STEPS = 6 };

template <typename T> static bool read_file(const char* path, std::vector<T>& v, size_t n)
{
    v.resize(n);
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    const size_t got = std::fread(v.data(), sizeof(T), n, f);
    std::fclose(f);
    return got == n;
}

// first record of the two that differ, or -1
template <typename T> static int first_diff(const std::vector<T>& a, const std::vector<T>& b, int n)
{
    for (int i = 0; i < n; ++i) if (std::memcmp(&a[i], &b[i], sizeof(T)) != 0) return i;
    return -1;
}

// Formulation B yardstick: records [0, batch) of d_src solved shard by shard on the plain handle
static int yard_b(ismpc_handle* h, int world, int batch, const ismpc_tick_in* d_src, ismpc_tick_out* d_tmp, std::vector<ismpc_tick_out>& ref)
{
    ref.assign((size_t)batch, ismpc_tick_out());
    int covered = 0;
    for (int r = 0; r < world; ++r) {
        int first, count;
        CHECK(ismpc_shard_range(batch, r, world, &first, &count) == ISMPC_OK && first == covered, "shard %d", r);
        covered += count;
        if (count == 0) continue;
        CHECK(ismpc_solve_batch_device(h, count, d_src + first, d_tmp, nullptr, nullptr) == ISMPC_OK, "yardstick shard %d", r);
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(&ref[first], d_tmp, sizeof(ismpc_tick_out) * (size_t)count, hipMemcpyDeviceToHost));
    }
    CHECK(covered == batch, "shards cover %d of %d", covered, batch);
    return 0;
}

// the gathered buffer `buf` of EVERY local device, read on a caller stream behind ismpc_group_wait_on, against `ref`
static int read_all(ismpc_group* g, int world, int batch, int buf, const std::vector<ismpc_tick_out>& ref, ismpc_tick_out* (*seen)[2], const char* what, int step)
{
    std::vector<ismpc_tick_out> got((size_t)batch);
    hipStream_t s; HIP_OK(hipStreamCreate(&s));
    for (int l = 0; l < world; ++l) {
        ismpc_tick_out* res = nullptr;
        CHECK(ismpc_group_result_device(g, l, buf, &res) == ISMPC_OK && res, "result_device local %d", l);
        if (seen) { if (!seen[l][buf]) seen[l][buf] = res; CHECK(seen[l][buf] == res, "%s step %d: the gathered buffer %d of local %d moved", what, step, buf, l); }
        std::memset(got.data(), 0xcd, sizeof(ismpc_tick_out) * (size_t)batch);
        CHECK(ismpc_group_wait_on(g, l, buf, s) == ISMPC_OK, "wait_on");
        HIP_OK(hipMemcpyAsync(got.data(), res, sizeof(ismpc_tick_out) * (size_t)batch, hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
        const int d = first_diff(got, ref, batch);
        CHECK(d < 0, "%s step %d, local device %d: record %d of %d differs from the per-shard yardstick", what, step, l, d, batch);
    }
    HIP_OK(hipStreamDestroy(s));
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 6) { std::fprintf(stderr, "usage\n"); return 2; }
    const int world = std::atoi(argv[1]);
    const bool ragged = std::getenv("ISMPC_GROUP_FORCE_RAGGED") != nullptr;
    CHECK(world >= 2 && world <= 8, "world %d", world);
    CHECK(ismpc_group_rccl_version() == 1, "the test double is not the bound RCCL: version %d", ismpc_group_rccl_version());

    std::vector<ismpc_tick_in> in;
    CHECK(read_file(argv[2], in, (size_t)B_MAX), "reading %s", argv[2]);
    std::vector<int> devices((size_t)world, 0);

    // ================================================== Formulation B ==================================================
    ismpc_params p; ismpc_params_default(&p);
    const int rows = 40;
    std::vector<double> ftsp((size_t)rows * 4, 0.0);
    for (int i = 1; i < rows; ++i) {
        ftsp[4 * i + 0] = (i - 1) * 0.2; ftsp[4 * i + 1] = ((i - 1) % 2 == 0 ? 1.0 : -1.0) * 0.08;
        ftsp[4 * i + 3] = (p.mpc_dt / p.control_dt) * (p.S + p.F) * i;
    }
    ismpc_handle* h = nullptr;
    CHECK(ismpc_create(&p, ftsp.data(), rows, 0, &h) == ISMPC_OK, "ismpc_create");
    ismpc_group* g = nullptr;
    CHECK(ismpc_group_create(&p, ftsp.data(), rows, devices.data(), world, &g) == ISMPC_OK, "ismpc_group_create on %d x device 0", world);
    CHECK(ismpc_group_world(g) == world && ismpc_group_local(g) == world, "world %d local %d", ismpc_group_world(g), ismpc_group_local(g));
    for (int k = 0; k < world; ++k) CHECK(ismpc_group_rank(g, k) == k && ismpc_group_handle(g, k) != nullptr, "rank of local %d", k);

    ismpc_tick_in* d_in = nullptr; ismpc_tick_out* d_tmp = nullptr;                  // the input twice in a row: step k reads records k .. k + batch - 1
    HIP_OK(hipMalloc((void**)&d_in, sizeof(ismpc_tick_in) * (size_t)B_MAX * 2));
    HIP_OK(hipMalloc((void**)&d_tmp, sizeof(ismpc_tick_out) * (size_t)B_MAX));
    std::vector<ismpc_tick_out> ref, out;

    // ---- host entry point: out_host is the concatenation of the per-shard yardsticks
    const int host_batches[3] = {4096, 4099, 5};
    for (int bi = 0; bi < (ragged ? 1 : 3); ++bi) {
        const int batch = host_batches[bi];
        HIP_OK(hipMemcpy(d_in, in.data(), sizeof(ismpc_tick_in) * (size_t)batch, hipMemcpyHostToDevice));
        if (yard_b(h, world, batch, d_in, d_tmp, ref)) return 1;
        out.assign((size_t)batch, ismpc_tick_out()); std::memset(out.data(), 0xab, sizeof(ismpc_tick_out) * (size_t)batch);
        CHECK(ismpc_group_solve_batch(g, batch, in.data(), out.data()) == ISMPC_OK, "ismpc_group_solve_batch(%d)", batch);
        const int d = first_diff(out, ref, batch);
        CHECK(d < 0, "solve_batch(%d): record %d differs from the per-shard yardstick", batch, d);
        if (read_all(g, world, batch, 0, ref, nullptr, "solve_batch", batch)) return 1;   // ... and every device holds all of it
    }

    // ---- the device path, double-buffered: 6 steps, the input of step k is the batch rotated by k records, read one step behind
    const int sb = ragged ? 4096 : B_MAX;
    HIP_OK(hipMemcpy(d_in, in.data(), sizeof(ismpc_tick_in) * (size_t)sb, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_in + sb, in.data(), sizeof(ismpc_tick_in) * (size_t)sb, hipMemcpyHostToDevice));
    std::vector<std::vector<ismpc_tick_out>> step_ref(STEPS);
    for (int k = 0; k < STEPS; ++k) if (yard_b(h, world, sb, d_in + k, d_tmp, step_ref[k])) return 1;
    CHECK(first_diff(step_ref[0], step_ref[1], sb) >= 0, "the steps' inputs do not differ: the test could not see a stale buffer");
    CHECK(ismpc_group_reserve(g, B_MAX) == ISMPC_OK, "reserve");
    ismpc_tick_out* seen[8][2] = {};
    for (int k = 0; k <= STEPS; ++k) {
        if (k < STEPS) {
            const ismpc_tick_in* shards[8] = {};
            for (int r = 0; r < world; ++r) { int first, count; ismpc_shard_range(sb, r, world, &first, &count); shards[r] = count ? d_in + k + first : nullptr; }
            CHECK(ismpc_group_step_device(g, sb, shards, k & 1) == ISMPC_OK, "step %d", k);
        }
        if (k >= 1 && read_all(g, world, sb, (k - 1) & 1, step_ref[k - 1], seen, "step_device", k - 1)) return 1;   // step k-1, while step k runs
    }
    CHECK(ismpc_group_sync(g) == ISMPC_OK, "sync");

    if (!ragged) {
        // ---- 5 instances: ranks 5..7 of 8 own nothing and pass NULL (2, 2, 1 at world 3)
        const int batch = 5;
        if (yard_b(h, world, batch, d_in + 7, d_tmp, ref)) return 1;
        const ismpc_tick_in* shards[8] = {};
        int empty = 0;
        for (int r = 0; r < world; ++r) { int first, count; ismpc_shard_range(batch, r, world, &first, &count); shards[r] = count ? d_in + 7 + first : nullptr; empty += count == 0; }
        CHECK(empty == (world > batch ? world - batch : 0), "%d empty ranks", empty);
        CHECK(ismpc_group_step_device(g, batch, shards, 1) == ISMPC_OK, "step_device(5)");
        if (read_all(g, world, batch, 1, ref, seen, "step_device(5)", 0)) return 1;
        CHECK(ismpc_group_sync(g) == ISMPC_OK, "sync");
    }
    ismpc_group_destroy(g); ismpc_destroy(h);
    HIP_OK(hipFree(d_in)); HIP_OK(hipFree(d_tmp));

    // ================================================== Formulation A ==================================================
    int a_cases = 0, a_ok = 0, a_ok_inst = 0;               // (instances whose tick ended ISMPC_A_ST_OK: reported, the comparison is on bytes whatever the status)
    if (!ragged) {
        std::vector<ismpc_a_state> st0; std::vector<double> push; std::vector<ismpc_a_inst> inst;
        CHECK(read_file(argv[3], st0, (size_t)A_MAX) && read_file(argv[4], push, (size_t)A_MAX * 2) && read_file(argv[5], inst, (size_t)A_MAX), "reading the A inputs");
        ismpc_a_params ap; ismpc_a_params_default(1, &ap);
        ismpc_a_gait gait[2]; ismpc_a_gait_default(1, 0.78539816339744828, 0.1, &gait[0]); ismpc_a_gait_default(1, 0.78539816339744828, 0.12, &gait[1]);
        std::vector<double> fp((size_t)(gait[0].n_gait + 1) * 8), ce[2];
        for (int k = 0; k < 2; ++k) { ce[k].resize((size_t)gait[k].n_gait * 2); CHECK(ismpc_a_plan(&gait[k], fp.data(), ce[k].data()) > 0, "ismpc_a_plan"); }
        ismpc_a_handle* ha = nullptr; ismpc_a_group* ga = nullptr;
        CHECK(ismpc_a_create(&ap, ce[0].data(), 0, &ha) == ISMPC_OK, "ismpc_a_create");
        CHECK(ismpc_a_group_create(&ap, ce[0].data(), devices.data(), world, &ga) == ISMPC_OK, "ismpc_a_group_create on %d x device 0", world);
        CHECK(ismpc_a_group_world(ga) == world && ismpc_a_group_local(ga) == world && ismpc_a_group_rank(ga, world - 1) == world - 1, "A world/local/rank");
        ismpc_a_state* d_st = nullptr; double* d_push = nullptr; ismpc_a_inst* d_inst = nullptr; ismpc_a_out* d_out = nullptr;
        HIP_OK(hipMalloc((void**)&d_st, sizeof(ismpc_a_state) * A_MAX)); HIP_OK(hipMalloc((void**)&d_push, 16 * A_MAX));
        HIP_OK(hipMalloc((void**)&d_inst, sizeof(ismpc_a_inst) * A_MAX)); HIP_OK(hipMalloc((void**)&d_out, sizeof(ismpc_a_out) * A_MAX));
        const int a_batches[2] = {768, 5};
        for (int with_inst = 0; with_inst < 2; ++with_inst) {
            if (with_inst) {   // per-instance records over two plans, solved in fp32
                CHECK(ismpc_a_add_plan(ha, ce[1].data()) == 1 && ismpc_a_group_add_plan(ga, ce[1].data()) == 1, "add_plan");
                CHECK(ismpc_a_set_precision(ha, 1) == ISMPC_OK && ismpc_a_group_set_precision(ga, 1) == ISMPC_OK, "set_precision");
            }
            for (int bi = 0; bi < 2; ++bi) {
                const int batch = a_batches[bi];
                std::vector<ismpc_a_out> aref((size_t)batch), aout((size_t)batch); std::vector<ismpc_a_state> sref((size_t)batch), sgot(st0.begin(), st0.begin() + batch);
                for (int r = 0; r < world; ++r) {        // the yardstick, shard by shard
                    int first, count; ismpc_shard_range(batch, r, world, &first, &count);
                    if (count == 0) continue;
                    HIP_OK(hipMemcpy(d_st, &st0[first], sizeof(ismpc_a_state) * (size_t)count, hipMemcpyHostToDevice));
                    HIP_OK(hipMemcpy(d_push, &push[2 * (size_t)first], 16 * (size_t)count, hipMemcpyHostToDevice));
                    HIP_OK(hipMemcpy(d_inst, &inst[first], sizeof(ismpc_a_inst) * (size_t)count, hipMemcpyHostToDevice));
                    CHECK((with_inst ? ismpc_a_tick_batch_inst_device(ha, count, d_st, d_inst, d_push, d_out, nullptr)
                                     : ismpc_a_tick_batch_device(ha, count, d_st, d_push, d_out, nullptr)) == ISMPC_OK, "A yardstick shard %d", r);
                    HIP_OK(hipDeviceSynchronize());
                    HIP_OK(hipMemcpy(&aref[first], d_out, sizeof(ismpc_a_out) * (size_t)count, hipMemcpyDeviceToHost));
                    HIP_OK(hipMemcpy(&sref[first], d_st, sizeof(ismpc_a_state) * (size_t)count, hipMemcpyDeviceToHost));
                }
                CHECK(first_diff(sref, sgot, batch) >= 0, "the tick does not move the state: the write-back could not be seen");
                std::memset(aout.data(), 0xab, sizeof(ismpc_a_out) * (size_t)batch);
                CHECK(ismpc_a_group_tick_batch(ga, batch, sgot.data(), with_inst ? inst.data() : nullptr, push.data(), aout.data()) == ISMPC_OK, "ismpc_a_group_tick_batch(%d)", batch);
                int d = first_diff(aout, aref, batch);
                CHECK(d < 0, "A batch %d inst %d: output record %d differs from the per-shard yardstick", batch, with_inst, d);
                d = first_diff(sgot, sref, batch);
                CHECK(d < 0, "A batch %d inst %d: written-back state %d differs from the per-shard yardstick", batch, with_inst, d);
                for (const ismpc_a_out& o : aref) (with_inst ? a_ok_inst : a_ok) += o.status == ISMPC_A_ST_OK;
                ++a_cases;
            }
        }
        ismpc_a_group_destroy(ga); ismpc_a_destroy(ha);
        HIP_OK(hipFree(d_st)); HIP_OK(hipFree(d_push)); HIP_OK(hipFree(d_inst)); HIP_OK(hipFree(d_out));
    }
    std::printf("OK world=%d double=%d ragged=%s steps=%d a_cases=%d a_ok=%d a_ok_inst=%d\n", world, ismpc_group_rccl_version(), ragged ? "forced" : "no", STEPS, a_cases, a_ok, a_ok_inst);
    return 0;
}
