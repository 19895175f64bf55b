// Filling and freeing a W4Device (w4_upload.h).  Host code over the HIP runtime: no kernel.
#include "w4_upload.h"

namespace fh {

void w4_free(W4Device& w) {
    if (w.qw) (void)hipFree(w.qw);
    if (w.sc) (void)hipFree(w.sc);
    if (w.zp) (void)hipFree(w.zp);
    if (w.perm) (void)hipFree(w.perm);
    if (w.inv_perm) (void)hipFree(w.inv_perm);
    if (w.bias) (void)hipFree(w.bias);
    if (w.f16t) (void)hipFree(w.f16t);
    w = W4Device();
}

int w4_upload(const W4HostPacked& hp, W4Device* w) {
    w4_free(*w);
    w4_set_dims(w, hp.k, hp.n, 1, false);
    FH_CHECK_HIP(hipMalloc((void**)&w->qw, hp.qw.size() * 4));
    FH_CHECK_HIP(hipMemcpy(w->qw, hp.qw.data(), hp.qw.size() * 4, hipMemcpyHostToDevice));
    FH_CHECK_HIP(hipMalloc((void**)&w->sc, hp.sc.size() * 2));
    FH_CHECK_HIP(hipMemcpy(w->sc, hp.sc.data(), hp.sc.size() * 2, hipMemcpyHostToDevice));
    if (!hp.symmetric) {
        FH_CHECK_HIP(hipMalloc((void**)&w->zp, hp.zp.size() * 2));
        FH_CHECK_HIP(hipMemcpy(w->zp, hp.zp.data(), hp.zp.size() * 2, hipMemcpyHostToDevice));
    }
    return hp.perm.empty() ? 0 : w4_upload_perm(hp.perm, w);
}

// input-column permutation of an act-order projection and its inverse (producers that scatter use the inverse)
int w4_upload_perm(const std::vector<int32_t>& perm, W4Device* w) {
    std::vector<int32_t> inv(perm.size());
    for (size_t j = 0; j < perm.size(); j++) inv[perm[j]] = (int32_t)j;
    FH_CHECK_HIP(hipMalloc((void**)&w->perm, perm.size() * 4));
    FH_CHECK_HIP(hipMemcpy(w->perm, perm.data(), perm.size() * 4, hipMemcpyHostToDevice));
    FH_CHECK_HIP(hipMalloc((void**)&w->inv_perm, inv.size() * 4));
    FH_CHECK_HIP(hipMemcpy(w->inv_perm, inv.data(), inv.size() * 4, hipMemcpyHostToDevice));
    return 0;
}

int w4_stack_reserve(W4Device* w, int k, int n, int E, bool fused) {
    if (w->qw) return 0;
    w4_set_dims(w, k, n, E, fused);
    FH_CHECK_HIP(hipMalloc((void**)&w->qw, w4_qw_words(w->n64, w->G) * 4 * E));
    FH_CHECK_HIP(hipMalloc((void**)&w->sc, w4_sc_elems(w->n64, w->G) * 2 * E));
    return 0;
}

// explicit zero points (asymmetric packs; cuda/quant.rs:795-839 sends those to the vLLM MoE lane): the array arrives with the
// first asymmetric expert, pre-filled with the implicit zero 8 of the symmetric experts written before and after it
int w4_stack_put(W4Device* w, int expert, const W4HostPacked& hp) {
    const size_t sc_elems = hp.sc.size();
    if (!hp.symmetric && !w->zp) {
        FH_CHECK_HIP(hipMalloc((void**)&w->zp, sc_elems * 2 * (size_t)w->num_experts));
        std::vector<uint16_t> eight(sc_elems * (size_t)w->num_experts, (uint16_t)0x4800);          // fp16 8.0
        FH_CHECK_HIP(hipMemcpy(w->zp, eight.data(), eight.size() * 2, hipMemcpyHostToDevice));
    }
    FH_CHECK_HIP(hipMemcpy(w->qw + (size_t)expert * hp.qw.size(), hp.qw.data(), hp.qw.size() * 4, hipMemcpyHostToDevice));
    FH_CHECK_HIP(hipMemcpy(w->sc + (size_t)expert * hp.sc.size(), hp.sc.data(), hp.sc.size() * 2, hipMemcpyHostToDevice));
    if (w->zp && !hp.symmetric)
        FH_CHECK_HIP(hipMemcpy(reinterpret_cast<uint16_t*>(w->zp) + (size_t)expert * sc_elems, hp.zp.data(), sc_elems * 2, hipMemcpyHostToDevice));
    return 0;
}

}  // namespace fh
