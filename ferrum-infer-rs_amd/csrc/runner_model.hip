// Decoder runner (C-ABI `ferrum_hip_model_*`), model build: create / destroy, the weight setters (uploads, GPTQ repack and the
// act-order folds), RoPE tables, synthetic weights, and finalize with every scratch allocation.  The sequence / KV calls are
// in runner_kv.hip, the forward in runner_forward.hip, its drivers in runner_steps.hip, tensor parallelism in runner_tp.hip.
#include <math.h>

#include "runner.h"
#include "knobs.h"
#include "tp_comm.h"
#include "w4_upload.h"

using namespace fh;

namespace {

int upload_f32_as_f16(const float* src, size_t n, __half** dst) {
    std::vector<uint16_t> tmp(n);
    for (size_t i = 0; i < n; i++) {
        _Float16 h = (_Float16)src[i];
        memcpy(&tmp[i], &h, 2);
    }
    if (!*dst) FH_CHECK_HIP(hipMalloc((void**)dst, n * 2));
    FH_CHECK_HIP(hipMemcpy(*dst, tmp.data(), n * 2, hipMemcpyHostToDevice));
    return 0;
}

// RoPE table (llama_family.rs:5220-5282): angle in f64, stored f32.
double rope_freq(const FerrumHipModelConfig& c, int i) {
    double base = 1.0 / pow(c.rope_theta, (double)(2 * i) / (double)c.head_dim);
    if (c.rope_scaling_kind == 1) return base / c.rope_p0;
    if (c.rope_scaling_kind == 2) {
        double wavelen = 2.0 * M_PI / base;
        double low_wl = c.rope_p3 / c.rope_p1, high_wl = c.rope_p3 / c.rope_p2;
        if (wavelen < high_wl) return base;
        if (wavelen > low_wl) return base / c.rope_p0;
        double smooth = (c.rope_p3 / wavelen - c.rope_p1) / (c.rope_p2 - c.rope_p1);
        return (1.0 - smooth) * base / c.rope_p0 + smooth * base;
    }
    return base;
}

// synthetic weights: counter-based hash RNG (splitmix64), reproducible for a given seed
__device__ __forceinline__ uint64_t splitmix(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
// packed INT4 words with zero-mean codes: nibble 0 is remapped to 8, so q − 8 ∈ [−7, 7] has mean 0
// (a non-zero mean would give every GEMM output a token-independent common mode and collapse the
// synthetic router onto a handful of experts — not the traffic pattern of a trained model).
__global__ void synth_u32_kernel(uint32_t* p, long n, uint64_t seed) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t w = (uint32_t)(splitmix(seed + (uint64_t)i) >> 16);
    uint32_t zero_nibbles = ~(w | (w >> 1) | (w >> 2) | (w >> 3)) & 0x11111111u;   // 1 where a nibble is 0
    p[i] = w | (zero_nibbles << 3);
}
__global__ void synth_f16_uniform_kernel(__half* p, long n, uint64_t seed, float lo, float hi) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        float u = (float)(splitmix(seed + (uint64_t)i) >> 40) / 16777216.0f;
        p[i] = __float2half(lo + u * (hi - lo));
    }
}
__global__ void synth_f16_normal_kernel(__half* p, long n, uint64_t seed, float std) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        uint64_t r = splitmix(seed + (uint64_t)i);
        float u1 = ((float)(r >> 40) + 0.5f) / 16777216.0f, u2 = (float)((r >> 16) & 0xFFFFFF) / 16777216.0f;
        p[i] = __float2half(std * sqrtf(-2.0f * logf(u1)) * cosf(6.2831853f * u2));
    }
}
__global__ void fill_f16_kernel(__half* p, long n, float v) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = __float2half(v);
}

int check_shape(const char* what, int k, int n, int ek, int en) {
    FH_REQUIRE(k == ek && n == en, "model_set_gptq(%s): got K=%d N=%d, config expects K=%d N=%d", what, k, n, ek, en);
    return 0;
}

}  // namespace

static int q_dim(const FerrumHipModelConfig& c) { return c.num_heads * c.head_dim; }
static int kv_dim(const FerrumHipModelConfig& c) { return c.num_kv_heads * c.head_dim; }
static int qkv_dim(const FerrumHipModelConfig& c) { return q_dim(c) + 2 * kv_dim(c); }

extern "C" {

int ferrum_hip_model_create(FerrumHipModel** model, const FerrumHipModelConfig* cfg) {
    FH_REQUIRE(model && cfg, "model_create: null argument");
    FH_REQUIRE(cfg->num_layers > 0 && cfg->hidden > 0 && cfg->hidden % 128 == 0, "model_create: hidden=%d must be a multiple of 128", cfg->hidden);
    FH_REQUIRE(cfg->num_kv_heads > 0 && cfg->num_heads % cfg->num_kv_heads == 0, "model_create: heads %d/%d", cfg->num_heads, cfg->num_kv_heads);
    FH_REQUIRE(cfg->num_heads / cfg->num_kv_heads <= 16, "model_create: GQA group %d > 16 unsupported", cfg->num_heads / cfg->num_kv_heads);
    FH_REQUIRE(cfg->head_dim == 64 || cfg->head_dim == 128 || cfg->head_dim == 256, "model_create: head_dim=%d unsupported", cfg->head_dim);
    FH_REQUIRE(cfg->max_seqs > 0 && cfg->max_tokens >= cfg->max_seqs && cfg->kv_num_blocks > 0 && cfg->max_seq_len > 0,
               "model_create: max_seqs/max_tokens/kv_num_blocks/max_seq_len must be positive");
    FH_REQUIRE(cfg->group_size > 0 && cfg->group_size % 128 == 0, "model_create: group_size=%d must be a multiple of 128", cfg->group_size);
    if (cfg->num_experts > 0) {
        FH_REQUIRE(cfg->top_k > 0 && cfg->top_k <= cfg->num_experts && cfg->num_experts <= 512, "model_create: experts=%d top_k=%d", cfg->num_experts, cfg->top_k);
        FH_REQUIRE(cfg->expert_inter % 128 == 0, "model_create: expert_inter=%d must be a multiple of 128", cfg->expert_inter);
    } else {
        FH_REQUIRE(cfg->intermediate > 0 && cfg->intermediate % 128 == 0, "model_create: intermediate=%d must be a multiple of 128", cfg->intermediate);
    }
    FH_REQUIRE(!cfg->sandwich_norms || cfg->num_experts == 0, "model_create: sandwich norms are implemented for dense MLP models");
    FH_REQUIRE(cfg->sliding_window_pattern >= 0 && cfg->rope_local_theta >= 0.0, "model_create: bad local-attention schedule");
    FH_REQUIRE(cfg->expert_parallel >= 0 && cfg->expert_parallel <= 2 && cfg->vocab_parallel >= 0 && cfg->vocab_parallel <= 1,
               "model_create: expert_parallel=%d vocab_parallel=%d", cfg->expert_parallel, cfg->vocab_parallel);
    if (cfg->expert_parallel && cfg->tp_world > 1) {
        FH_REQUIRE(cfg->num_experts > 0 && cfg->num_experts % cfg->tp_world == 0, "model_create: expert_parallel needs num_experts (%d) divisible by the world size (%d)",
                   cfg->num_experts, cfg->tp_world);
    }
    auto* m = new FerrumHipModel();
    m->cfg = *cfg;
    if (m->cfg.tp_world < 1) { m->cfg.tp_world = 1; m->cfg.tp_rank = 0; }
    if (m->cfg.tp_world == 1) { m->cfg.expert_parallel = 0; m->cfg.vocab_parallel = 0; }
    m->vp_n = m->cfg.vocab;
    if (m->cfg.vocab_parallel) {
        const int per = (cdiv(m->cfg.vocab, m->cfg.tp_world) + 15) / 16 * 16;       // whole 16-row tiles per rank
        m->vp_v0 = std::min(m->cfg.vocab, m->cfg.tp_rank * per);
        m->vp_n = std::min(m->cfg.vocab, m->vp_v0 + per) - m->vp_v0;
        FH_REQUIRE(m->vp_n > 0, "model_create: vocab_parallel leaves rank %d of %d without vocabulary rows (V=%d)", m->cfg.tp_rank, m->cfg.tp_world, m->cfg.vocab);
    }
    m->ep_E = m->cfg.num_experts;
    if (m->cfg.expert_parallel) {
        m->ep_E = m->cfg.num_experts / m->cfg.tp_world;
        m->ep_e0 = m->cfg.tp_rank * m->ep_E;
    }
    m->layers.resize(cfg->num_layers);
    m->max_blocks_per_seq = cdiv(cfg->max_seq_len, KV_BLOCK);
    hipError_t e = hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete m; fh::set_error("model_create: hipStreamCreate: %s", hipGetErrorString(e)); return 1; }
    // RoPE tables: the main one (θ, optional scaling) and, for Gemma-3 style models, the unscaled local-layer table
    const int half = cfg->head_dim / 2;
    auto build_table = [&](bool local, float** cos_d, float** sin_d) -> bool {
        std::vector<float> cs((size_t)cfg->max_seq_len * half), sn((size_t)cfg->max_seq_len * half);
        std::vector<double> freq(half);
        for (int i = 0; i < half; i++)
            freq[i] = local ? 1.0 / pow(cfg->rope_local_theta, (double)(2 * i) / (double)cfg->head_dim) : rope_freq(*cfg, i);
        for (int pos = 0; pos < cfg->max_seq_len; pos++)
            for (int i = 0; i < half; i++) {
                double ang = (double)pos * freq[i];
                cs[(size_t)pos * half + i] = (float)cos(ang);
                sn[(size_t)pos * half + i] = (float)sin(ang);
            }
        if (hipMalloc((void**)cos_d, cs.size() * 4) != hipSuccess || hipMalloc((void**)sin_d, sn.size() * 4) != hipSuccess) return false;
        (void)hipMemcpy(*cos_d, cs.data(), cs.size() * 4, hipMemcpyHostToDevice);
        (void)hipMemcpy(*sin_d, sn.data(), sn.size() * 4, hipMemcpyHostToDevice);
        return true;
    };
    if (!build_table(false, &m->cos_t, &m->sin_t) || (cfg->rope_local_theta > 0.0 && !build_table(true, &m->cos_local, &m->sin_local))) {
        fh::set_error("model_create: rope table allocation failed");
        ferrum_hip_model_destroy(m);
        return 1;
    }
    m->seqs.reset(new SeqTable((uint32_t)cfg->kv_num_blocks, KV_BLOCK, m->max_blocks_per_seq));
    if (const char* e = getenv("FERRUM_HIP_ROUTE_PARTS")) m->route_parts = std::max(1, atoi(e));
    if (const char* e = getenv("FERRUM_HIP_FUSE_TAIL_ROWS")) m->fuse_tail_max_rows = std::max(0, std::min(4, atoi(e)));
    if (const char* e = getenv("FERRUM_HIP_FUSE_ROPE")) m->fuse_rope_attn = atoi(e) != 0;
    if (const char* e = getenv("FERRUM_HIP_O_SLABS")) m->o_slabs = std::max(0, atoi(e));
    if (const char* e = getenv("FERRUM_HIP_DENSE_SLABS")) m->dense_slabs = atoi(e) != 0;
    if (const char* e = getenv("FERRUM_HIP_ROUTE_GEMM_TOKENS")) m->route_gemm_min_tokens = std::max(1, atoi(e));
    if (const char* e = getenv("FERRUM_HIP_MOE_TILE_PAIRS")) m->moe_tile_min_pairs_per_expert = std::max(1, atoi(e));
    if (const char* e = getenv("FERRUM_HIP_MOE_EM_PAIRS")) m->moe_em_min_pairs_x8 = 8 * std::max(0, atoi(e));
    if (const char* e = getenv("FERRUM_HIP_MOE_EM_PAIRS_X8")) m->moe_em_min_pairs_x8 = std::max(0, atoi(e));
    if (knobs().attn_flash_min_rows_set) m->attn_flash_min_rows = std::max(1, (int)knobs().attn_flash_min_rows);   // as the launcher reads it
    if (const char* e = getenv("FERRUM_HIP_MOE_TILE96_PAIRS")) m->moe_tile96_min_pairs_per_expert = std::max(1, atoi(e));
    if (const char* e = getenv("FERRUM_HIP_MOE_TILE128_PAIRS")) m->moe_tile128_min_pairs_per_expert = std::max(1, atoi(e));
    if (const char* e = getenv("FERRUM_HIP_MOE_TILE32_PAIRS")) m->moe_tile32_min_pairs_per_expert = std::max(1, atoi(e));
    *model = m;
    return 0;
}

int ferrum_hip_model_destroy(FerrumHipModel* m) {
    if (!m) return 0;
    drop_graph(m);
    if (m->comm && m->comm_owned) ferrum_hip_comm_destroy(m->comm);
    for (auto& L : m->layers) {
        for (__half* p : {L.input_ln, L.post_ln, L.q_norm, L.k_norm, L.router, L.k_pool, L.v_pool, L.post_attn_ln, L.post_ffn_ln, L.qkv_bias})
            if (p) (void)hipFree(p);
        w4_free(L.qkv); w4_free(L.o); w4_free(L.gate_up); w4_free(L.down); w4_free(L.exp_gate_up); w4_free(L.exp_down);
    }
    for (void* p : {(void*)m->embed, (void*)m->lm_head, (void*)m->lm_head_t, (void*)m->final_norm, (void*)m->cos_t, (void*)m->sin_t,
                    (void*)m->residual, (void*)m->norm_out, (void*)m->qkv_out, (void*)m->q_out, (void*)m->attn_out,
                    (void*)m->o_out, (void*)m->gate_up_out, (void*)m->act_out, (void*)m->mlp_out,
                    (void*)m->sampled_hidden, (void*)m->moe_act, (void*)m->moe_down, (void*)m->moe_gather_x, (void*)m->moe_gather_h, (void*)m->router_logits,
                    (void*)m->expert_ids, (void*)m->sorted_ids, (void*)m->block_ids, (void*)m->total_post_pad,
                    (void*)m->expert_w, (void*)m->logits, (void*)m->out_tokens, (void*)m->workspace, (void*)m->taps,
                    (void*)m->idx_dev, (void*)m->history, (void*)m->step_counter, (void*)m->residual2, (void*)m->chain_o_part, (void*)m->chain_attn_partial, (void*)m->chain_attn_tickets,
                    (void*)m->route_cand, (void*)m->route_stats, (void*)m->route_arrive, (void*)m->cos_local,
                    (void*)m->sin_local, (void*)m->residual_f32, (void*)m->gather_scratch, (void*)m->greedy_opts_dev, (void*)m->tp_tmp,
                    (void*)m->expert_ids_local, (void*)m->ones, m->vp_pairs, m->vp_gathered,
                    (void*)m->kv_pools_dev, (void*)m->kv_pairs_dev, (void*)m->kv_staging, (void*)m->embed_out,
                    (void*)m->score_hidden, (void*)m->score_logits, (void*)m->score_lists, (void*)m->score_results})
        if (p) (void)hipFree(p);
    if (m->idx_host) (void)hipHostFree(m->idx_host);
    if (m->inlaunch_timeouts) (void)hipHostFree(m->inlaunch_timeouts);
    if (m->stream) (void)hipStreamDestroy(m->stream);
    delete m;
    return 0;
}

int ferrum_hip_model_set_global_f32(FerrumHipModel* m, int which, const float* data) {
    FH_REQUIRE(m && data, "model_set_global: null argument");
    const size_t vh = (size_t)m->cfg.vocab * m->cfg.hidden;
    switch (which) {
    case 0: return upload_f32_as_f16(data, vh, &m->embed);
    case 1: return upload_f32_as_f16(data, vh, &m->lm_head);
    case 2: return upload_f32_as_f16(data, m->cfg.hidden, &m->final_norm);
    }
    fh::set_error("model_set_global: which=%d", which);
    return FERRUM_HIP_INVALID;
}

int ferrum_hip_model_set_layer_dense_f32(FerrumHipModel* m, int layer, int which, const float* data) {
    FH_REQUIRE(m && data && layer >= 0 && layer < m->cfg.num_layers, "model_set_layer_dense: bad argument");
    LayerWeights& L = m->layers[layer];
    switch (which) {
    case 0: return upload_f32_as_f16(data, m->cfg.hidden, &L.input_ln);
    case 1: return upload_f32_as_f16(data, m->cfg.hidden, &L.post_ln);
    case 2: return upload_f32_as_f16(data, m->cfg.head_dim, &L.q_norm);
    case 3: return upload_f32_as_f16(data, m->cfg.head_dim, &L.k_norm);
    case 4:
        FH_REQUIRE(m->cfg.num_experts > 0, "model_set_layer_dense: router on a dense model");
        return upload_f32_as_f16(data, (size_t)m->cfg.num_experts * m->cfg.hidden, &L.router);
    case 7:   // fused q|k|v projection bias (Qwen2 family, gptq.rs:56): attached to the qkv GEMM at finalize
        return upload_f32_as_f16(data, (size_t)qkv_dim(m->cfg), &L.qkv_bias);
    case 5: return upload_f32_as_f16(data, m->cfg.hidden, &L.post_attn_ln);
    case 6: return upload_f32_as_f16(data, m->cfg.hidden, &L.post_ffn_ln);
    }
    fh::set_error("model_set_layer_dense: which=%d", which);
    return FERRUM_HIP_INVALID;
}

// Dense gate_up: when down is act-order (perm P: down reads act'[j] = act[P[j]]), pack column j of the gate half from the
// checkpoint's gate column P[j] and column I + j from up column I + P[j]: the gated activation of the packed output IS act'.
static int pack_gate_up(FerrumHipModel* m, LayerWeights& L, const int32_t* qweight, const float* scales, const int32_t* qzeros,
                        const int32_t* g_idx, int k, int n) {
    W4HostPacked hp;
    std::vector<int32_t> cols;
    const std::vector<int32_t>& P = L.down_perm_host;
    const int I = n / 2;
    const bool fold = !P.empty() && (int)P.size() == I && L.down.qw != nullptr;
    if (fold) {
        cols.resize(n);
        for (int j = 0; j < I; j++) { cols[j] = P[j]; cols[I + j] = I + P[j]; }
    }
    if (int r = w4_repack_host(qweight, scales, qzeros, g_idx, fold ? cols.data() : nullptr, m->cfg.group_size, k, n, &hp)) return r;
    if (int r = w4_upload(hp, &L.gate_up)) return r;
    L.down.perm_folded = fold;
    return 0;
}

int ferrum_hip_model_set_gptq(FerrumHipModel* m, int layer, int which, int expert, const int32_t* qweight,
                              const float* scales, const int32_t* qzeros, const int32_t* g_idx, int k, int n) {
    FH_REQUIRE(m && qweight && scales && qzeros && layer >= 0 && layer < m->cfg.num_layers, "model_set_gptq: bad argument");
    const FerrumHipModelConfig& c = m->cfg;
    LayerWeights& L = m->layers[layer];
    W4HostPacked hp;
    const int H = c.hidden;
    if (which <= 3) {
        int rc = 0;
        W4Device* dst = nullptr;
        switch (which) {
        case 0: rc = check_shape("qkv", k, n, H, qkv_dim(c)); dst = &L.qkv; break;
        case 1: rc = check_shape("o", k, n, q_dim(c), H); dst = &L.o; break;
        case 2: rc = check_shape("gate_up", k, n, H, 2 * c.intermediate); dst = &L.gate_up; break;
        case 3: rc = check_shape("down", k, n, c.intermediate, H); dst = &L.down; break;
        }
        if (rc) return rc;
        if (which == 2 && !L.down_set) {
            // down has not arrived: if it turns out to be act-order, its row permutation becomes the column order of gate_up
            // (the gated activation then leaves already permuted — no gather in front of down) — wait for it
            auto p = std::make_unique<LayerWeights::PendingGptq>();
            const int groups = k / c.group_size;
            p->qweight.assign(qweight, qweight + (size_t)(k / 8) * n);
            p->scales.assign(scales, scales + (size_t)groups * n);
            p->qzeros.assign(qzeros, qzeros + (size_t)groups * (n / 8));
            p->has_g_idx = g_idx != nullptr;
            if (g_idx) p->g_idx.assign(g_idx, g_idx + k);
            p->k = k; p->n = n;
            L.pending_gate_up = std::move(p);
            return 0;
        }
        if (which == 2) return pack_gate_up(m, L, qweight, scales, qzeros, g_idx, k, n);
        if (int r = w4_repack_host(qweight, scales, qzeros, g_idx, nullptr, c.group_size, k, n, &hp)) return r;
        if (int r = w4_upload(hp, dst)) return r;
        if (which == 3) {
            L.down_set = true;
            L.down_perm_host = hp.perm;
            if (L.pending_gate_up) {
                std::unique_ptr<LayerWeights::PendingGptq> p = std::move(L.pending_gate_up);
                return pack_gate_up(m, L, p->qweight.data(), p->scales.data(), p->qzeros.data(), p->has_g_idx ? p->g_idx.data() : nullptr, p->k, p->n);
            }
        }
        return 0;
    }
    FH_REQUIRE(which == 4 || which == 5, "model_set_gptq: which=%d", which);
    FH_REQUIRE(c.num_experts > 0 && expert >= 0 && expert < c.num_experts, "model_set_gptq: expert=%d of %d", expert, c.num_experts);
    if (expert < m->ep_e0 || expert >= m->ep_e0 + m->ep_E) return 0;     // expert parallel: another rank's expert (a loader may offer all of them)
    expert -= m->ep_e0;
    const bool gu = which == 4;
    if (int rc = gu ? check_shape("expert gate_up", k, n, H, 2 * c.expert_inter) : check_shape("expert down", k, n, c.expert_inter, H)) return rc;
    std::vector<int32_t> perm;
    if (gu) perm = gate_up_col_perm(n);
    // act-order (desc_act) expert stacks (cuda/quant.rs:862 ff.): the packed rows are sorted by quant group, and — as the reference
    // takes ONE g_idx for a stack (capabilities.rs:180-189: the experts share their K-axis quantisation) — every expert must
    // bring the same row permutation; the grouped GEMMs then read gathered input rows (moe_gemm_inputs below).
    if (int r = w4_repack_host(qweight, scales, qzeros, g_idx, gu ? perm.data() : nullptr, c.group_size, k, n, &hp)) return r;
    W4Device* w = gu ? &L.exp_gate_up : &L.exp_down;
    std::vector<int32_t>& perm_host = gu ? L.exp_gate_up_perm_host : L.exp_down_perm_host;
    const bool first = L.exp_loaded.empty() || std::none_of(L.exp_loaded.begin(), L.exp_loaded.end(), [&](uint8_t b) { return (b & (gu ? 1 : 2)) != 0; });
    if (int rc = w4_stack_reserve(w, k, n, m->ep_E, gu)) return rc;
    if (first) {
        perm_host = hp.perm;
        if (!hp.perm.empty())
            if (int rc = w4_upload_perm(hp.perm, w)) return rc;
    } else {
        FH_REQUIRE(perm_host == hp.perm, "model_set_gptq: layer %d expert %d %s brings a different g_idx than the experts before it (a stack shares one)",
                   layer, expert + m->ep_e0, gu ? "gate_up" : "down");
    }
    if (int rc = w4_stack_put(w, expert, hp)) return rc;
    if (L.exp_loaded.empty()) L.exp_loaded.assign(m->ep_E, 0);
    L.exp_loaded[expert] |= gu ? 1 : 2;
    return 0;
}

// Unquantised projection (DenseLinear, ferrum-kernels/src/linear.rs:109-129): W [n, k] row-major f32 on the host → fp16
// f16t tiles on the device; the forward then runs it through the fp16 GEMM (B::gemm).  which: 0 qkv, 1 o, 2 gate_up, 3 down.
int ferrum_hip_model_set_dense_f32(FerrumHipModel* m, int layer, int which, const float* weight, int k, int n) {
    FH_REQUIRE(m && weight && !m->finalized && layer >= 0 && layer < m->cfg.num_layers, "model_set_dense: bad argument");
    const FerrumHipModelConfig& c = m->cfg;
    LayerWeights& L = m->layers[layer];
    const int H = c.hidden;
    int rc = 0;
    W4Device* dst = nullptr;
    switch (which) {
    case 0: rc = check_shape("qkv", k, n, H, qkv_dim(c)); dst = &L.qkv; break;
    case 1: rc = check_shape("o", k, n, q_dim(c), H); dst = &L.o; break;
    case 2: rc = check_shape("gate_up", k, n, H, 2 * c.intermediate); dst = &L.gate_up; break;
    case 3: rc = check_shape("down", k, n, c.intermediate, H); dst = &L.down; break;
    default: fh::set_error("model_set_dense: which=%d", which); return FERRUM_HIP_INVALID;
    }
    if (rc) return rc;
    FH_REQUIRE(k % 32 == 0, "model_set_dense: K=%d must be a multiple of 32", k);
    w4_free(*dst);
    w4_set_dims(dst, k, n, 1, false);
    __half* row = nullptr;
    if (int r = upload_f32_as_f16(weight, (size_t)n * k, &row)) return r;
    hipError_t e = hipMalloc((void**)&dst->f16t, f16t_elems(n, k) * 2);
    if (e != hipSuccess) { (void)hipFree(row); fh::set_error("model_set_dense: hipMalloc: %s", hipGetErrorString(e)); return 1; }
    rc = f16t_repack(row, dst->f16t, n, k, m->stream);
    (void)hipStreamSynchronize(m->stream);
    (void)hipFree(row);
    return rc;
}

static void launch1d(void (*k)(__half*, long, uint64_t, float, float), __half* p, long n, uint64_t seed, float a, float b, hipStream_t s) {
    hipLaunchKernelGGL(k, dim3(cdiv(n, 256)), dim3(256), 0, s, p, n, seed, a, b);
}

// Synthetic weights generated on the device (bench only: no checkpoints are available offline).
// qweight nibbles uniform, scales uniform [0.01,0.1)·f with f = 1/(0.25·sqrt(K)) so that
// dequantised W has std ≈ 1/sqrt(K) and activations stay O(1) through all layers,
// zero point 8 (sym), norm weights 1, embeddings / lm_head / router N(0, 0.02).
static int synth_w4(W4Device* w, int k, int n, int E, bool fused, uint64_t seed, hipStream_t s) {
    w4_free(*w);
    w4_set_dims(w, k, n, E, fused);
    long qw = (long)w4_qw_words(w->n64, w->G) * E, sc = (long)w4_sc_elems(w->n64, w->G) * E;
    FH_CHECK_HIP(hipMalloc((void**)&w->qw, qw * 4));
    FH_CHECK_HIP(hipMalloc((void**)&w->sc, sc * 2));
    hipLaunchKernelGGL(synth_u32_kernel, dim3(cdiv(qw, 256)), dim3(256), 0, s, w->qw, qw, seed);
    float f = 1.0f / (0.25f * sqrtf((float)k));   // std(q-8)·mean(scale) ≈ 4.5·0.055
    launch1d(synth_f16_uniform_kernel, w->sc, sc, seed ^ 0x5ca1e5ull, 0.01f * f, 0.1f * f, s);
    FH_CHECK_LAUNCH();
    return 0;
}

int ferrum_hip_model_init_synthetic(FerrumHipModel* m, uint64_t seed) {
    FH_REQUIRE(m && !m->finalized, "model_init_synthetic: bad state");
    const FerrumHipModelConfig& c = m->cfg;
    hipStream_t s = m->stream;
    auto alloc_fill = [&](__half** p, long n, float v) -> int {
        if (!*p) FH_CHECK_HIP(hipMalloc((void**)p, n * 2));
        hipLaunchKernelGGL(fill_f16_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, *p, n, v);
        return 0;
    };
    auto alloc_normal = [&](__half** p, long n, uint64_t sd, float std) -> int {
        if (!*p) FH_CHECK_HIP(hipMalloc((void**)p, n * 2));
        hipLaunchKernelGGL(synth_f16_normal_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, *p, n, sd, std);
        return 0;
    };
    const long vh = (long)c.vocab * c.hidden;
    if (int rc = alloc_normal(&m->embed, vh, seed ^ 0xe0bedull, 0.02f)) return rc;
    if (int rc = alloc_normal(&m->lm_head, vh, seed ^ 0x1a4eadull, 0.02f)) return rc;
    if (int rc = alloc_fill(&m->final_norm, c.hidden, 1.0f)) return rc;
    for (int li = 0; li < c.num_layers; li++) {
        LayerWeights& L = m->layers[li];
        // replicated tensors (router, norms) come from the layer seed; the sharded projections of a tensor-parallel rank
        // additionally mix in the rank, so every rank holds its own slice-shaped weights while embed / lm_head / norms /
        // router agree across ranks (all ranks then sample the same token from identical all-reduced activations)
        const uint64_t ls0 = seed + 0x1000003ull * (uint64_t)(li + 1);
        const uint64_t ls = ls0 + 0x51ed270bull * (uint64_t)(c.tp_world > 1 ? c.tp_rank : 0);
        if (int rc = alloc_fill(&L.input_ln, c.hidden, 1.0f)) return rc;
        if (int rc = alloc_fill(&L.post_ln, c.hidden, 1.0f)) return rc;
        if (c.sandwich_norms) {
            if (int rc = alloc_fill(&L.post_attn_ln, c.hidden, 1.0f)) return rc;
            if (int rc = alloc_fill(&L.post_ffn_ln, c.hidden, 1.0f)) return rc;
        }
        if (c.has_qk_norm) {
            if (int rc = alloc_fill(&L.q_norm, c.head_dim, 1.0f)) return rc;
            if (int rc = alloc_fill(&L.k_norm, c.head_dim, 1.0f)) return rc;
        }
        if (int rc = synth_w4(&L.qkv, c.hidden, qkv_dim(c), 1, false, ls ^ 0x11, s)) return rc;
        if (int rc = synth_w4(&L.o, q_dim(c), c.hidden, 1, false, ls ^ 0x22, s)) return rc;
        if (c.num_experts > 0) {
            if (int rc = alloc_normal(&L.router, (long)c.num_experts * c.hidden, ls0 ^ 0x33, 0.02f)) return rc;
            if (int rc = synth_w4(&L.exp_gate_up, c.hidden, 2 * c.expert_inter, m->ep_E, true, ls ^ 0x44, s)) return rc;
            if (int rc = synth_w4(&L.exp_down, c.expert_inter, c.hidden, m->ep_E, false, ls ^ 0x55, s)) return rc;
            L.exp_loaded.assign(m->ep_E, 3);
        } else {
            if (int rc = synth_w4(&L.gate_up, c.hidden, 2 * c.intermediate, 1, false, ls ^ 0x44, s)) return rc;
            if (int rc = synth_w4(&L.down, c.intermediate, c.hidden, 1, false, ls ^ 0x55, s)) return rc;
        }
    }
    // development (FERRUM_HIP_SYNTH_DESC_ACT=1): give every dense projection an activation-order permutation, as a desc_act GPTQ
    // checkpoint has (BASELINE configs[3]) — the weights are random anyway; what this reproduces is the cost of serving the
    // permuted inputs (producers write them permuted; prefill o_proj keeps one gather launch)
    if (const char* e = getenv("FERRUM_HIP_SYNTH_DESC_ACT"); e && atoi(e)) {
        for (int li = 0; li < c.num_layers; li++) {
            LayerWeights& L = m->layers[li];
            for (W4Device* w : {&L.qkv, &L.o, &L.gate_up, &L.down}) {
                if (!w->qw || w->perm) continue;
                std::vector<int32_t> perm(w->k);
                for (int i = 0; i < w->k; i++) perm[i] = i;
                uint64_t st = seed ^ (0x9e3779b97f4a7c15ull * (uint64_t)(li * 8 + (w - &L.qkv) + 1));
                for (int i = w->k - 1; i > 0; i--) {          // Fisher–Yates with the reference's LCG
                    st = st * 6364136223846793005ull + 1442695040888963407ull;
                    std::swap(perm[i], perm[(int)((st >> 33) % (uint64_t)(i + 1))]);
                }
                if (int rc = w4_upload_perm(perm, w)) return rc;
            }
            // (random weights: a gate_up whose columns were packed in down's row order is just another random matrix)
            L.down.perm_folded = L.down.perm && L.gate_up.qw;
        }
    }
    FH_CHECK_HIP(hipStreamSynchronize(s));
    return 0;
}

int ferrum_hip_model_finalize(FerrumHipModel* m) {
    FH_REQUIRE(m, "model_finalize: null");
    if (m->finalized) return 0;
    const FerrumHipModelConfig& c = m->cfg;
    FH_REQUIRE(m->embed && m->final_norm, "model_finalize: embed / final_norm missing");
    for (LayerWeights& L : m->layers)
        if (L.pending_gate_up) {      // down never arrived as GPTQ (unquantised, or missing: reported below): nothing to fold
            std::unique_ptr<LayerWeights::PendingGptq> p = std::move(L.pending_gate_up);
            if (int rc = pack_gate_up(m, L, p->qweight.data(), p->scales.data(), p->qzeros.data(), p->has_g_idx ? p->g_idx.data() : nullptr, p->k, p->n))
                return rc;
        }
    for (int li = 0; li < c.num_layers; li++) {
        const LayerWeights& L = m->layers[li];
        auto have = [](const W4Device& w) { return w.qw != nullptr || w.f16t != nullptr; };
        FH_REQUIRE(L.input_ln && L.post_ln && have(L.qkv) && have(L.o), "model_finalize: layer %d attention weights missing", li);
        FH_REQUIRE(!c.has_qk_norm || (L.q_norm && L.k_norm), "model_finalize: layer %d q/k norm missing", li);
        FH_REQUIRE(!c.sandwich_norms || (L.post_attn_ln && L.post_ffn_ln), "model_finalize: layer %d sandwich norms missing", li);
        if (m->layers[li].qkv_bias) {    // the GEMM epilogue / split-K reduce adds it (W4Device::bias owns it from here)
            m->layers[li].qkv.bias = m->layers[li].qkv_bias;
            m->layers[li].qkv_bias = nullptr;
        }
        if (c.num_experts > 0) {
            FH_REQUIRE(L.router && L.exp_gate_up.qw && L.exp_down.qw, "model_finalize: layer %d MoE weights missing", li);
            for (int e = 0; e < m->ep_E; e++)
                FH_REQUIRE(L.exp_loaded[e] == 3, "model_finalize: layer %d expert %d incomplete", li, e + m->ep_e0);
        } else {
            FH_REQUIRE(have(L.gate_up) && have(L.down), "model_finalize: layer %d MLP weights missing", li);
        }
    }
    const size_t T = c.max_tokens, S = c.max_seqs, H = c.hidden;
    // dense fp16 weights that are streamed every step → fragment-major tiles (f16t)
    {
        const __half* head = m->lm_head ? m->lm_head : m->embed;     // tied lm_head (llama_family.rs:969-1001)
        // vocabulary parallel: only this rank's rows [vp_v0, vp_v0 + vp_n) become tiles
        FH_CHECK_HIP(hipMalloc((void**)&m->lm_head_t, f16t_elems(m->vp_n, c.hidden) * 2));
        if (int rc = f16t_repack(head + (size_t)m->vp_v0 * c.hidden, m->lm_head_t, m->vp_n, c.hidden, m->stream)) return rc;
        if (m->lm_head) {
            FH_CHECK_HIP(hipStreamSynchronize(m->stream));
            (void)hipFree(m->lm_head);
            m->lm_head = nullptr;
        }
        for (auto& L : m->layers)
            if (L.router) {
                __half* t = nullptr;
                FH_CHECK_HIP(hipMalloc((void**)&t, f16t_elems(c.num_experts, c.hidden) * 2));
                if (int rc = f16t_repack(L.router, t, c.num_experts, c.hidden, m->stream)) return rc;
                FH_CHECK_HIP(hipStreamSynchronize(m->stream));
                (void)hipFree(L.router);
                L.router = t;
            }
    }
    // KV pools, zero-initialised
    for (auto& L : m->layers) {
        size_t elems = (size_t)c.kv_num_blocks * c.num_kv_heads * kv_tile_elems(c.head_dim);
        if (int rc = dev_alloc(&L.k_pool, elems)) return rc;
        if (int rc = dev_alloc(&L.v_pool, elems)) return rc;
    }
    {   // the pools as one device pointer array (K0, V0, K1, V1, …): what a whole-block KV move indexes by grid row
        std::vector<void*> pools;
        for (auto& L : m->layers) { pools.push_back(L.k_pool); pools.push_back(L.v_pool); }
        FH_CHECK_HIP(hipMalloc((void**)&m->kv_pools_dev, pools.size() * sizeof(void*)));
        FH_CHECK_HIP(hipMemcpy(m->kv_pools_dev, pools.data(), pools.size() * sizeof(void*), hipMemcpyHostToDevice));
    }
    int rc = 0;
    rc |= dev_alloc(&m->residual, T * H);
    if (c.sandwich_norms) rc |= dev_alloc(&m->residual_f32, T * H);
    {
        size_t kmax = 0;     // act-order input gather scratch
        for (const LayerWeights& L : m->layers)
            for (const W4Device* w : {&L.qkv, &L.o, &L.gate_up, &L.down})
                if (w->perm && !w->perm_folded) kmax = std::max(kmax, (size_t)w->k);
        if (kmax) rc |= dev_alloc(&m->gather_scratch, T * kmax);
    }
    rc |= dev_alloc(&m->norm_out, T * H);
    rc |= dev_alloc(&m->qkv_out, T * qkv_dim(c));
    rc |= dev_alloc(&m->q_out, T * q_dim(c));
    rc |= dev_alloc(&m->attn_out, T * q_dim(c));
    rc |= dev_alloc(&m->o_out, T * H);
    rc |= dev_alloc(&m->mlp_out, T * H);
    rc |= dev_alloc(&m->sampled_hidden, S * H);
    rc |= dev_alloc(&m->logits, S * (size_t)m->vp_n);
    if (c.vocab_parallel) {
        FH_CHECK_HIP(hipMalloc(&m->vp_pairs, S * 8));
        FH_CHECK_HIP(hipMalloc(&m->vp_gathered, S * 8 * (size_t)c.tp_world));
    }
    rc |= dev_alloc(&m->out_tokens, S);
    if (c.num_experts > 0) {
        const size_t P = T * c.top_k, sorted_max = P + (size_t)c.num_experts * 128;  // room for 128-row blocks (prefill)
        rc |= dev_alloc(&m->router_logits, T * c.num_experts);
        rc |= dev_alloc(&m->expert_ids, P);
        if (c.expert_parallel) {
            rc |= dev_alloc(&m->expert_ids_local, P);
            if (!rc) {
                FH_CHECK_HIP(hipMalloc((void**)&m->ones, T * sizeof(float)));
                std::vector<float> one(T, 1.0f);
                FH_CHECK_HIP(hipMemcpy(m->ones, one.data(), T * sizeof(float), hipMemcpyHostToDevice));
            }
        }
        rc |= dev_alloc(&m->expert_w, P);
        rc |= dev_alloc(&m->sorted_ids, sorted_max);
        rc |= dev_alloc(&m->block_ids, sorted_max / 16 + 1);
        rc |= dev_alloc(&m->total_post_pad, (size_t)4);
        rc |= dev_alloc(&m->residual2, (size_t)128 * H);
        // the router's candidate lists: [T][Q][8] and [T][Q][2] — every form that writes them checks T · Q against the capacity
        // (the split route kernel: ≤ 64 rows of ≤ 8 parts; the chain's deferred forms: moe_deferred_merge_ok, moe_pair_rank_lists_ok)
        rc |= dev_alloc(&m->route_cand, (size_t)MOE_ROUTE_LIST_CAPACITY * 8);
        rc |= dev_alloc(&m->route_stats, (size_t)MOE_ROUTE_LIST_CAPACITY * 2);
        // [64] arrival counters of the split route kernel (zeroed here; the kernel re-arms them) + [2][E] per-expert counters of the
        // merged gate_up → down launch + its give-up count; the head kernel of every forward zeroes the route counters and half 0
        // layout: route [64] | pair half 0 | chain half 0 | pair half 1 | chain half 1
        m->arrive_half_words = (size_t)c.num_experts * MOE_PAIR_COUNTER_STRIDE + decode_chain_counter_words();
        rc |= dev_alloc(&m->route_arrive, (size_t)64 + 2 * m->arrive_half_words + 4);
        if (!rc) m->em2_arrive = m->route_arrive + 64;
        if (!rc) {
            FH_CHECK_HIP(hipHostMalloc((void**)&m->inlaunch_timeouts, 64, hipHostMallocDefault));
            *m->inlaunch_timeouts = 0u;
        }
        rc |= dev_alloc(&m->moe_act, P * c.expert_inter);
        rc |= dev_alloc(&m->moe_down, P * H);
        bool gx_perm = false, dn_perm = false;                  // act-order expert stacks: gathered GEMM inputs
        for (const LayerWeights& L : m->layers) { gx_perm |= L.exp_gate_up.perm != nullptr; dn_perm |= L.exp_down.perm != nullptr; }
        if (gx_perm) rc |= dev_alloc(&m->moe_gather_x, T * H);
        if (dn_perm) rc |= dev_alloc(&m->moe_gather_h, P * c.expert_inter);
    } else {
        rc |= dev_alloc(&m->gate_up_out, T * 2 * c.intermediate);
        rc |= dev_alloc(&m->act_out, T * (size_t)c.intermediate);
        // the one-launch attention half of the decode layer (chain.hip) for dense models: ping-pong residual, its two counter halves
        // (layout as above without the per-expert part) and the give-up word
        rc |= dev_alloc(&m->residual2, (size_t)128 * H);
        m->arrive_half_words = (size_t)decode_chain_counter_words();
        rc |= dev_alloc(&m->route_arrive, (size_t)64 + 2 * m->arrive_half_words + 4);
        if (!rc) m->em2_arrive = m->route_arrive + 64;
        if (!rc) {
            FH_CHECK_HIP(hipHostMalloc((void**)&m->inlaunch_timeouts, 64, hipHostMallocDefault));
            *m->inlaunch_timeouts = 0u;
        }
    }
    if (!rc && m->em2_arrive) rc |= dev_alloc(&m->chain_o_part, (size_t)4 * 128 * H);
    if (!rc && m->em2_arrive && c.head_dim == 128) {
        rc |= dev_alloc(&m->chain_attn_partial, (size_t)CHAIN_MAX_ATTN_WGS * 16 * (c.head_dim + 4));
        rc |= dev_alloc(&m->chain_attn_tickets, (size_t)4096);
    }
    if (rc) return rc;
    // workspace: split-K slabs (≤ 64 rows) and split-KV attention partials
    size_t widest = std::max<size_t>({(size_t)qkv_dim(c), (size_t)H, (size_t)2 * std::max(c.intermediate, 1), (size_t)c.vocab});
    size_t gemm_ws = (size_t)64 * 64 * ((widest + 63) / 64 * 64) * sizeof(float);
    size_t attn_ws = (size_t)32 * S * c.num_kv_heads * 16 * (c.head_dim + 2) * sizeof(float) * 2;
    m->workspace_bytes = std::max(gemm_ws, attn_ws);
    FH_CHECK_HIP(hipMalloc((void**)&m->workspace, m->workspace_bytes));
    // index block
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
    m->il.tokens = take(T * 4);
    m->il.cu_seqlens = take((S + 1) * 4);
    m->il.pos_offsets = take(S * 4);
    m->il.kv_lens = take(S * 4);
    m->il.sampled_idx = take(S * 4);
    m->il.embed_spans = take(S * 8);
    m->il.block_tables = take(S * m->max_blocks_per_seq * 4);
    m->il.total = off;
    FH_CHECK_HIP(hipHostMalloc((void**)&m->idx_host, off, hipHostMallocDefault));
    FH_CHECK_HIP(hipMalloc((void**)&m->idx_dev, off));
    FH_CHECK_HIP(hipMemset(m->idx_dev, 0, off));
    if (int r = dev_alloc(&m->step_counter, (size_t)4)) return r;
    m->finalized = true;
    return 0;
}

int ferrum_hip_model_stream(FerrumHipModel* m, void** stream) {
    FH_REQUIRE(m && stream, "model_stream: null");
    *stream = m->stream;
    return 0;
}

int ferrum_hip_model_local_vocab(const FerrumHipModel* m, int* vocab_start, int* vocab_count) {
    FH_REQUIRE(m, "model_local_vocab: null");
    if (vocab_start) *vocab_start = m->vp_v0;
    if (vocab_count) *vocab_count = m->vp_n;
    return 0;
}

}  // extern "C"
