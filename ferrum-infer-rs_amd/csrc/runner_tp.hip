// Decoder runner, tensor parallelism: the collectives the forward calls (RCCL / one-shot transport through tp_comm.hip, or the
// in-process host-barrier loopback of the tests) and the calls that give a model its communicator.
#include "runner.h"
#include "knobs.h"
#include "tp_comm.h"

#include <condition_variable>
#include <mutex>

using namespace fh;

namespace {
// Σ over ranks in rank order, fp32 accumulate, one rounding — every rank computes the same bits
__global__ void loopback_sum_kernel(const __half* const* bufs, int world, __half* out, long n) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int r = 0; r < world; r++) s += __half2float(bufs[r][i]);
    out[i] = __float2half(s);
}
}  // namespace

// In-process stand-in for the RCCL communicator (tests): the ranks of one tensor-parallel group are runner models driven
// by threads of ONE process on one GPU; an all-reduce is two host barriers around a device-side sum.  It validates the
// runner's sharded forward (column-parallel qkv / gate_up, row-parallel o / down, kv heads split) end to end where only
// one GPU exists; production uses ferrum_hip_model_tp_init (RCCL over xGMI).
struct FerrumHipTpLoopback {
    int world = 0;
    std::mutex mu;
    std::condition_variable cv;
    int arrived = 0;
    long generation = 0;
    const __half* bufs[8] = {};
    const __half** bufs_dev = nullptr;
    void barrier() {
        std::unique_lock<std::mutex> lk(mu);
        const long gen = generation;
        if (++arrived == world) { arrived = 0; generation++; cv.notify_all(); }
        else cv.wait(lk, [&] { return generation != gen; });
    }
};

namespace {
int loopback_all_reduce(FerrumHipModel* m, __half* buf, size_t count) {
    FerrumHipTpLoopback* lb = m->tp_loopback;
    if (int rc = grow_device((void**)&m->tp_tmp, &m->tp_tmp_bytes, count * 2, m->stream)) return rc;
    FH_CHECK_HIP(hipStreamSynchronize(m->stream));             // this rank's partial is complete
    { std::lock_guard<std::mutex> lk(lb->mu); lb->bufs[m->cfg.tp_rank] = buf; }
    lb->barrier();                                             // every partial is complete and published
    if (m->cfg.tp_rank == 0)
        FH_CHECK_HIP(hipMemcpy((void*)lb->bufs_dev, lb->bufs, sizeof(void*) * lb->world, hipMemcpyHostToDevice));
    lb->barrier();
    hipLaunchKernelGGL(loopback_sum_kernel, dim3(cdiv((long)count, 256)), dim3(256), 0, m->stream, lb->bufs_dev, lb->world, m->tp_tmp,
                       (long)count);
    FH_CHECK_LAUNCH();
    FH_CHECK_HIP(hipStreamSynchronize(m->stream));
    lb->barrier();                                             // everyone has read every partial
    FH_CHECK_HIP(hipMemcpyAsync(buf, m->tp_tmp, count * 2, hipMemcpyDeviceToDevice, m->stream));
    return 0;
}

// small all-gather through the host-barrier loopback (tests): out[world][bytes] in rank order
int loopback_all_gather(FerrumHipModel* m, const void* in, void* out, size_t bytes) {
    FerrumHipTpLoopback* lb = m->tp_loopback;
    FH_CHECK_HIP(hipStreamSynchronize(m->stream));
    { std::lock_guard<std::mutex> lk(lb->mu); lb->bufs[m->cfg.tp_rank] = reinterpret_cast<const __half*>(in); }
    lb->barrier();
    for (int p = 0; p < lb->world; p++)
        FH_CHECK_HIP(hipMemcpyAsync((uint8_t*)out + (size_t)p * bytes, lb->bufs[p], bytes, hipMemcpyDeviceToDevice, m->stream));
    FH_CHECK_HIP(hipStreamSynchronize(m->stream));
    lb->barrier();
    return 0;
}
}  // namespace

int fh::tp_all_gather(FerrumHipModel* m, const void* in, void* out, size_t bytes) {
    if (m->tp_loopback) { form_hit(FORM_TP_ALLREDUCE_LOOPBACK); return loopback_all_gather(m, in, out, bytes); }
    FH_REQUIRE(m->comm, "vocabulary parallel: no communicator (ferrum_hip_model_tp_init / ferrum_hip_model_set_comm)");
    return comm_all_gather_bytes(m->comm, in, out, bytes, m->stream);
}

int fh::tp_all_reduce(FerrumHipModel* m, __half* buf, size_t count) {
    if (m->cfg.tp_world <= 1) return 0;
    if (m->tp_loopback) { form_hit(FORM_TP_ALLREDUCE_LOOPBACK); return loopback_all_reduce(m, buf, count); }
    FH_REQUIRE(m->comm, "tensor parallel: no communicator (ferrum_hip_model_tp_init / ferrum_hip_model_set_comm)");
    return comm_all_reduce_f16(m->comm, buf, count, m->stream);
}

// residual += all_reduce(x); out = rms_norm(residual)·w (tp_decode.rs:350-372 + the layer's add + norm): ONE launch where the
// one-shot transport carries the message, else the all-reduce and fused_add_rms_norm_f16 — the same bits either way.
int fh::tp_all_reduce_add_rms_norm(FerrumHipModel* m, __half* x, __half* residual, const __half* w, float eps, __half* out, int T, int H,
                                   hipStream_t s, const int32_t* out_perm) {
    if (m->cfg.tp_world > 1 && !m->tp_loopback && m->comm && !out_perm) {
        int fused = 0;
        if (int rc = comm_all_reduce_add_rms_norm_f16(m->comm, x, residual, w, eps, out, T, H, &fused, s)) return rc;
        if (fused) return 0;
    }
    if (int rc = tp_all_reduce(m, x, (size_t)T * H)) return rc;
    return fused_add_rms_norm_f16(residual, x, w, eps, out, T, H, s, out_perm);
}

extern "C" {

int ferrum_hip_tp_loopback_create(FerrumHipTpLoopback** out, int world) {
    FH_REQUIRE(out && world >= 2 && world <= 8, "tp_loopback_create: world=%d", world);
    auto* lb = new FerrumHipTpLoopback();
    lb->world = world;
    if (hipMalloc((void**)&lb->bufs_dev, sizeof(void*) * 8) != hipSuccess) { delete lb; fh::set_error("tp_loopback_create: hipMalloc"); return 1; }
    *out = lb;
    return 0;
}
int ferrum_hip_tp_loopback_destroy(FerrumHipTpLoopback* lb) {
    if (lb) { (void)hipFree((void*)lb->bufs_dev); delete lb; }
    return 0;
}
int ferrum_hip_model_tp_attach_loopback(FerrumHipModel* m, FerrumHipTpLoopback* lb) {
    FH_REQUIRE(m && lb && m->cfg.tp_world == lb->world && m->cfg.tp_rank < lb->world, "tp_attach_loopback: world mismatch");
    m->tp_loopback = lb;
    return 0;
}

// RCCL rank of this model's tensor-parallel group (nccl_comm.rs:21-49): the communicator is owned by the model.
int ferrum_hip_model_tp_init(FerrumHipModel* m, const uint8_t id[128]) {
    FH_REQUIRE(m && id, "tp_init: null");
    if (m->cfg.tp_world <= 1) return 0;
    FerrumHipComm* c = nullptr;
    if (int rc = ferrum_hip_comm_create_rccl(&c, m->cfg.tp_world, m->cfg.tp_rank, id)) return rc;
    if (m->comm && m->comm_owned) ferrum_hip_comm_destroy(m->comm);
    m->comm = c;
    m->comm_owned = true;
    m->graph_refused = false;
    drop_graph(m);
    return 0;
}

// Attach a communicator created by the caller (ferrum_hip_comm_create_*); the model does not own it.  Also the way to
// re-read the all-reduce policy after ferrum_hip_debug_reload_knobs: a captured decode graph is dropped here.
int ferrum_hip_model_set_comm(FerrumHipModel* m, FerrumHipComm* comm) {
    FH_REQUIRE(m, "model_set_comm: null model");
    FH_REQUIRE(!comm || (ferrum_hip_comm_world_size(comm) == m->cfg.tp_world && ferrum_hip_comm_rank(comm) == m->cfg.tp_rank),
               "model_set_comm: communicator is rank %d of %d, model is rank %d of %d", comm ? ferrum_hip_comm_rank(comm) : 0,
               comm ? ferrum_hip_comm_world_size(comm) : 1, m->cfg.tp_rank, m->cfg.tp_world);
    if (m->comm && m->comm_owned) ferrum_hip_comm_destroy(m->comm);
    m->comm = comm;
    m->comm_owned = false;
    m->graph_refused = false;
    drop_graph(m);
    return 0;
}

}  // extern "C"
