// Decoder runner, the drivers of the forward: ferrum_hip_model_unified_forward{,_ex} (admission, index block, one forward),
// ferrum_hip_model_embed (the same forward with the embedding tail in place of the sampling head), ferrum_hip_model_score (… with
// the scoring head in its place),
// ferrum_hip_model_decode_steps (the steady-state decode loop: one step captured into a hipGraph and replayed) and the bench's
// ferrum_hip_model_time_kernel.
#include "runner.h"
#include "knobs.h"
#include "score_plan.h"
#include "tp_comm.h"

using namespace fh;

// ── tiny device helpers of the decode loop ──────────────────────────────────
// After a decode step: record the sampled tokens, feed them back as the next inputs, advance the
// per-sequence positions.  Everything the next step needs lives in device buffers, so one captured
// step can be replayed (the reference keeps per-iter state in buffers for the same reason,
// kernels/split_qkv_norm_rope_into_paged_cache.cu:9-16).
static __global__ void decode_advance_kernel(const uint32_t* __restrict__ sampled, uint32_t* __restrict__ tokens,
                                             uint32_t* __restrict__ pos_offsets, uint32_t* __restrict__ kv_lens,
                                             uint32_t* __restrict__ history, int32_t* __restrict__ step_counter, int n) {
    int i = threadIdx.x + blockIdx.x * blockDim.x;
    int step = *step_counter;
    if (i < n) {
        uint32_t t = sampled[i];
        tokens[i] = t;
        pos_offsets[i] += 1;
        kv_lens[i] += 1;
        history[(long)step * n + i] = t;
    }
    __syncthreads();
    if (i == 0) *step_counter = step + 1;
}

void fh::drop_graph(FerrumHipModel* m) {
    if (m->graph_exec) { (void)hipGraphExecDestroy(m->graph_exec); m->graph_exec = nullptr; }
    if (m->graph) { (void)hipGraphDestroy(m->graph); m->graph = nullptr; }
}

// Merged launches hand data over between workgroups and bound every wait; a wait that gave up has produced garbage.  Called
// after every host synchronisation of a forward: the call fails, the captured graph is dropped and the merged forms stay off.
int fh::check_inlaunch_waits(FerrumHipModel* m) {
    // tensor / expert / vocabulary parallel: a one-shot all-reduce or all-gather whose wait for a peer gave up left the rank's
    // un-reduced partial in the output — ids sampled from it must not be handed back as a success
    if (const unsigned n = comm_take_timeouts(m->comm)) {
        drop_graph(m);
        fh::set_error("%u one-shot collective call(s) gave up waiting for a peer: the results of this call are invalid; the one-shot "
                      "transport is off from now on (RCCL, where the communicator has a rank)", n);
        return 3;
    }
    if (!m->inlaunch_timeouts) return 0;
    const unsigned now = *reinterpret_cast<volatile unsigned*>(m->inlaunch_timeouts);
    if (now == m->inlaunch_timeouts_seen) return 0;
    const unsigned n = now - m->inlaunch_timeouts_seen;
    m->inlaunch_timeouts_seen = now;
    m->em2_failed = true;
    drop_graph(m);
    const unsigned n_pair = n & 0xffffu, n_chain = n >> 16;
    fh::set_error("in-launch waits of the merged kernels gave up — w4_gemm_moe_em2_kernel (gate_up → down hand-off): %u, "
                  "decode_chain_kernel (role hand-offs): %u: the results of this call are invalid; the multi-launch layer is used "
                  "from now on", n_pair, n_chain);
    return 3;
}
// one sequence's row of the host block table, padded with 0 (paged_pool.rs:438-440)
static void fill_block_table_row(const FerrumHipModel* m, int32_t* row, const SeqState& st) {
    for (int b = 0; b < m->max_blocks_per_seq; b++) row[b] = b < (int)st.blocks.size() ? (int32_t)st.blocks[b] : 0;
}

// The front of a forward over batch items (ferrum_hip_model_unified_forward_ex, ferrum_hip_model_embed): argument checks, the
// step's shape, KV admission, the index block (tokens, cu_seqlens, positions, kv lengths, sampled rows, the final-chunk items'
// row spans, block tables) filled and sent.  `who` names the entry point in the messages.
static int admit_and_upload(FerrumHipModel* m, const FerrumHipBatchItem* items, int num_items, const char* who, StepShape* shape) {
    FH_REQUIRE(items, "%s: null items", who);
    const FerrumHipModelConfig& c = m->cfg;
    FH_REQUIRE(num_items <= c.max_seqs, "%s: %d items > max_seqs %d", who, num_items, c.max_seqs);
    // shape + admission
    StepShape sh{};
    sh.num_seqs = num_items;
    sh.pure_decode = true;
    std::vector<FerrumHipKvSlotRequest> reqs(num_items);
    for (int i = 0; i < num_items; i++) {
        const FerrumHipBatchItem& it = items[i];
        FH_REQUIRE(it.num_q_tokens > 0 && it.q_tokens, "%s: item %d has no tokens", who, i);
        const int have = m->seqs->len(it.seq_id);
        FH_REQUIRE(it.pos_offset == have, "%s: item %d pos_offset=%d but cache holds %d tokens", who, i, it.pos_offset, have);
        FH_REQUIRE(it.pos_offset + it.num_q_tokens <= c.max_seq_len, "%s: item %d exceeds max_seq_len %d", who, i, c.max_seq_len);
        for (int t = 0; t < it.num_q_tokens; t++)
            FH_REQUIRE(it.q_tokens[t] < (uint32_t)c.vocab, "%s: item %d token %u out of vocab", who, i, it.q_tokens[t]);
        sh.m_total += it.num_q_tokens;
        sh.max_q_len = std::max(sh.max_q_len, it.num_q_tokens);
        sh.max_kv_len = std::max(sh.max_kv_len, it.pos_offset + it.num_q_tokens);
        if (it.num_q_tokens != 1) sh.pure_decode = false;
        if (it.is_final_chunk) sh.num_sampled++;
        reqs[i] = {it.seq_id, it.pos_offset + it.num_q_tokens, 0};
    }
    FH_REQUIRE(sh.m_total <= c.max_tokens, "%s: %d tokens > max_tokens %d", who, sh.m_total, c.max_tokens);
    sh.all_single_token = sh.pure_decode;
    if (c.sliding_window > 0 && c.sliding_window_pattern == 0) sh.pure_decode = false;   // uniform window: no full-attention layer
    if (int rc = m->seqs->reserve(reqs.data(), num_items, nullptr)) return rc;

    // index block
    const IndexBlock h = index_block(m, m->idx_host);
    int t = 0, j = 0;
    for (int i = 0; i < num_items; i++) {
        const FerrumHipBatchItem& it = items[i];
        h.cu[i] = (uint32_t)t;
        memcpy(h.tokens + t, it.q_tokens, (size_t)it.num_q_tokens * 4);
        t += it.num_q_tokens;
        h.pos[i] = (uint32_t)it.pos_offset;
        h.kvl[i] = (uint32_t)(it.pos_offset + it.num_q_tokens);
        if (it.is_final_chunk) {
            h.embed_spans[2 * j] = t - it.num_q_tokens;
            h.embed_spans[2 * j + 1] = t;
            h.sampled_idx[j++] = t - 1;
        }
        fill_block_table_row(m, h.bt + (size_t)i * m->max_blocks_per_seq, *m->seqs->find(it.seq_id));
    }
    h.cu[num_items] = (uint32_t)t;
    sh.single_prefix = 0;
    while (sh.single_prefix < num_items && items[sh.single_prefix].num_q_tokens == 1) sh.single_prefix++;
    sh.rest_min_q = 0;
    for (int i = sh.single_prefix; i < num_items; i++)
        sh.rest_min_q = i == sh.single_prefix ? items[i].num_q_tokens : std::min(sh.rest_min_q, items[i].num_q_tokens);
    // only the used prefix of the block-table region needs to travel
    size_t used = m->il.block_tables + (size_t)num_items * m->max_blocks_per_seq * 4;
    FH_CHECK_HIP(hipMemcpyAsync(m->idx_dev, m->idx_host, used, hipMemcpyHostToDevice, m->stream));
    *shape = sh;
    return 0;
}

extern "C" {

int ferrum_hip_model_unified_forward(FerrumHipModel* m, const FerrumHipBatchItem* items, int num_items, int greedy,
                                     uint32_t* out_tokens, float* logits_out) {
    return ferrum_hip_model_unified_forward_ex(m, items, num_items, greedy, nullptr, out_tokens, logits_out);
}

int ferrum_hip_model_unified_forward_ex(FerrumHipModel* m, const FerrumHipBatchItem* items, int num_items, int greedy,
                                        const FerrumHipGreedyOptions* opts, uint32_t* out_tokens, float* logits_out) {
    FH_REQUIRE(m && m->finalized, "unified_forward: model not finalized");
    if (num_items <= 0) return 0;
    StepShape sh{};
    if (int rc = admit_and_upload(m, items, num_items, "unified_forward", &sh)) return rc;
    GreedyDeviceOpts g{};
    if (greedy && opts && sh.num_sampled > 0) {
        // device copies of the greedy options live in a growable side buffer: [mask | row_offsets | token_ids | penalties]
        size_t total_ids = 0;
        if (opts->penalty_row_offsets) {
            FH_REQUIRE(opts->penalty_token_ids && opts->penalties, "unified_forward: incomplete repetition-penalty arrays");
            FH_REQUIRE(opts->penalty_row_offsets[0] == 0, "unified_forward: penalty_row_offsets must start at 0");
            for (int i = 0; i < sh.num_sampled; i++)
                FH_REQUIRE(opts->penalty_row_offsets[i + 1] >= opts->penalty_row_offsets[i], "unified_forward: penalty_row_offsets not monotone");
            total_ids = opts->penalty_row_offsets[sh.num_sampled];
        }
        const size_t mask_bytes = opts->valid_token_mask ? ((size_t)opts->mask_len + 15) / 16 * 16 : 0;
        const size_t off_ro = mask_bytes, off_ids = off_ro + ((size_t)sh.num_sampled + 1 + 3) / 4 * 16;
        const size_t off_pen = off_ids + (total_ids + 3) / 4 * 16, need = off_pen + ((size_t)sh.num_sampled + 3) / 4 * 16;
        if (int rc = grow_device((void**)&m->greedy_opts_dev, &m->greedy_opts_bytes, need, m->stream)) return rc;
        uint8_t* base = m->greedy_opts_dev;
        if (opts->valid_token_mask) {
            FH_REQUIRE(opts->mask_len > 0, "unified_forward: mask_len=%d", opts->mask_len);
            FH_CHECK_HIP(hipMemcpyAsync(base, opts->valid_token_mask, (size_t)opts->mask_len, hipMemcpyHostToDevice, m->stream));
            g.mask = base;
            g.mask_len = opts->mask_len;
        }
        if (opts->penalty_row_offsets) {
            FH_CHECK_HIP(hipMemcpyAsync(base + off_ro, opts->penalty_row_offsets, ((size_t)sh.num_sampled + 1) * 4, hipMemcpyHostToDevice, m->stream));
            if (total_ids)
                FH_CHECK_HIP(hipMemcpyAsync(base + off_ids, opts->penalty_token_ids, total_ids * 4, hipMemcpyHostToDevice, m->stream));
            FH_CHECK_HIP(hipMemcpyAsync(base + off_pen, opts->penalties, (size_t)sh.num_sampled * 4, hipMemcpyHostToDevice, m->stream));
            g.row_offsets = reinterpret_cast<const uint32_t*>(base + off_ro);
            g.token_ids = reinterpret_cast<const uint32_t*>(base + off_ids);
            g.penalties = reinterpret_cast<const float*>(base + off_pen);
        }
    }
    if (int rc = enqueue_forward(m, sh, greedy != 0, &g)) return rc;
    if (sh.num_sampled > 0) {
        if (greedy && out_tokens)
            FH_CHECK_HIP(hipMemcpyAsync(out_tokens, m->out_tokens, (size_t)sh.num_sampled * 4, hipMemcpyDeviceToHost, m->stream));
        if (logits_out)
            FH_CHECK_HIP(hipMemcpyAsync(logits_out, m->logits, (size_t)sh.num_sampled * m->vp_n * 4, hipMemcpyDeviceToHost, m->stream));
    }
    FH_CHECK_HIP(hipStreamSynchronize(m->stream));
    for (int i = 0; i < num_items; i++) m->seqs->advance(items[i].seq_id, items[i].num_q_tokens);
    return check_inlaunch_waits(m);
}

int ferrum_hip_model_embedding_dim(const FerrumHipModel* m, int* hidden) {
    FH_REQUIRE(m && hidden, "model_embedding_dim: null");
    *hidden = m->cfg.hidden;
    return 0;
}

int ferrum_hip_model_embed(FerrumHipModel* m, const FerrumHipBatchItem* items, int num_items, const FerrumHipEmbedOptions* opts,
                           float* out_host) {
    FH_REQUIRE(m && m->finalized, "model_embed: model not finalized");
    const FerrumHipModelConfig& c = m->cfg;
    const FerrumHipEmbedOptions o = opts ? *opts : FerrumHipEmbedOptions{0, 1, 0, 0, 0, 0};
    // pre-flight: nothing is reserved or launched for a request that cannot be served
    FH_REQUIRE(o.pooling >= 0 && o.pooling <= 2, "model_embed: pooling=%d must be 0 (last), 1 (mean) or 2 (first)", o.pooling);
    FH_REQUIRE(o.dims >= 0 && o.dims <= c.hidden, "model_embed: dims=%d must be 0 (all) or in [1, hidden=%d]", o.dims, c.hidden);
    if (num_items <= 0) return 0;
    FH_REQUIRE(items, "model_embed: null items");
    int num_final = 0;
    for (int i = 0; i < num_items; i++) {
        if (!items[i].is_final_chunk) continue;
        num_final++;
        FH_REQUIRE(o.pooling == 0 || items[i].pos_offset == 0,
                   "model_embed: item %d (sequence %llu) ends its sequence at pos_offset=%d: %s pooling needs the whole sequence in this "
                   "forward (only last-token pooling works over chunks or a cached prefix)",
                   i, (unsigned long long)items[i].seq_id, items[i].pos_offset, o.pooling == 1 ? "mean" : "first-token");
    }
    FH_REQUIRE(num_final == 0 || out_host, "model_embed: null output");
    if (int rc = grow_device((void**)&m->embed_out, &m->embed_out_bytes, (size_t)c.max_seqs * c.hidden * sizeof(float), m->stream)) return rc;
    StepShape sh{};
    if (int rc = admit_and_upload(m, items, num_items, "model_embed", &sh)) return rc;
    const int d = o.dims ? o.dims : c.hidden;
    const EmbedHead eh{o.pooling, o.normalize != 0, o.dims, o.skip_final_norm == 0, sh.max_q_len, m->embed_out};
    if (int rc = enqueue_forward(m, sh, false, nullptr, nullptr, nullptr, &eh)) return rc;
    if (num_final > 0)
        FH_CHECK_HIP(hipMemcpyAsync(out_host, m->embed_out, (size_t)num_final * d * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    FH_CHECK_HIP(hipStreamSynchronize(m->stream));
    for (int i = 0; i < num_items; i++) m->seqs->advance(items[i].seq_id, items[i].num_q_tokens);
    const int rc = check_inlaunch_waits(m);
    if (o.release)
        for (int i = 0; i < num_items; i++)
            if (items[i].is_final_chunk) (void)ferrum_hip_model_release(m, items[i].seq_id);
    return rc;
}

int ferrum_hip_model_score(FerrumHipModel* m, const FerrumHipBatchItem* items, int num_items, const FerrumHipScoreTarget* targets,
                           int num_targets, const FerrumHipScoreOptions* opts, FerrumHipTokenScore* out_host) {
    FH_REQUIRE(m && m->finalized, "model_score: model not finalized");
    const FerrumHipModelConfig& c = m->cfg;
    if (c.vocab_parallel) {
        fh::set_error("model_score: a vocabulary-parallel lm_head is not scored (the log-sum-exp of a sharded row needs a merge across ranks)");
        return 3;
    }
    const FerrumHipScoreOptions o = opts ? *opts : FerrumHipScoreOptions{0, 0};
    // pre-flight: nothing is reserved or launched for a request that cannot be served
    FH_REQUIRE(num_items <= 0 || items, "model_score: null items");
    FH_REQUIRE(num_targets <= 0 || targets, "model_score: null targets");
    FH_REQUIRE(num_targets <= 0 || out_host, "model_score: null output with %d targets", num_targets);
    std::vector<int32_t> item_rows(std::max(num_items, 0));
    for (int i = 0; i < num_items; i++) item_rows[i] = items[i].num_q_tokens;
    std::vector<ScoreTargetRef> refs(std::max(num_targets, 0));
    for (int t = 0; t < num_targets; t++) refs[t] = {targets[t].item, targets[t].row, targets[t].token};
    ScoreBatchPlan plan;
    char why[256];
    if (score_batch_plan(ScoreBatchShape{num_items, item_rows.data(), num_targets, refs.data(), c.vocab, c.hidden, c.max_tokens, o.max_rows_per_pass},
                         &plan, why, sizeof(why))) {
        fh::set_error("%s", why);
        return 2;
    }
    FH_REQUIRE(plan.workspace_bytes <= m->workspace_bytes, "model_score: a pass of %d rows needs a workspace of %zu bytes, the model has %zu",
               plan.pass_rows, plan.workspace_bytes, m->workspace_bytes);
    if (num_items == 0) return 0;
    const int T = num_targets, R = plan.num_rows;
    if (T > 0) {
        if (int rc = grow_device((void**)&m->score_hidden, &m->score_hidden_bytes, plan.hidden_bytes, m->stream)) return rc;
        if (int rc = grow_device((void**)&m->score_logits, &m->score_logits_bytes, plan.logits_bytes, m->stream)) return rc;
        if (int rc = grow_device((void**)&m->score_lists, &m->score_lists_bytes, plan.lists_bytes, m->stream)) return rc;
        if (int rc = grow_device((void**)&m->score_results, &m->score_results_bytes, plan.results_bytes, m->stream)) return rc;
    }
    StepShape sh{};
    if (int rc = admit_and_upload(m, items, num_items, "model_score", &sh)) return rc;
    std::vector<float> results((size_t)T + 2 * (size_t)R);      // pair log-probs [T] | row top log-probs [R] | row top tokens [R]
    ScoreHead head{};
    if (T > 0) {
        int32_t* lists = m->score_lists;                         // rows [R] | pair_rows [T] | pair_tokens [T]
        FH_CHECK_HIP(hipMemcpyAsync(lists, plan.rows.data(), (size_t)R * 4, hipMemcpyHostToDevice, m->stream));
        FH_CHECK_HIP(hipMemcpyAsync(lists + R, plan.pair_rows.data(), (size_t)T * 4, hipMemcpyHostToDevice, m->stream));
        FH_CHECK_HIP(hipMemcpyAsync(lists + R + T, plan.pair_tokens.data(), (size_t)T * 4, hipMemcpyHostToDevice, m->stream));
        head = ScoreHead{plan.num_passes, plan.pass_row_begin.data(), plan.pass_pair_begin.data(), lists, lists + R,
                         reinterpret_cast<const uint32_t*>(lists + R + T), m->score_results, m->score_results + T,
                         reinterpret_cast<uint32_t*>(m->score_results + T + R)};
    }
    if (int rc = enqueue_forward(m, sh, false, nullptr, nullptr, nullptr, nullptr, &head)) return rc;
    if (T > 0) FH_CHECK_HIP(hipMemcpyAsync(results.data(), m->score_results, results.size() * 4, hipMemcpyDeviceToHost, m->stream));
    FH_CHECK_HIP(hipStreamSynchronize(m->stream));
    for (int i = 0; i < num_items; i++) m->seqs->advance(items[i].seq_id, items[i].num_q_tokens);
    const int rc = check_inlaunch_waits(m);
    for (int t = 0; t < T; t++) {
        const int r = plan.target_pass[t] * plan.pass_rows + plan.target_pass_row[t];
        uint32_t top;
        memcpy(&top, &results[(size_t)T + R + r], 4);
        out_host[t] = FerrumHipTokenScore{results[plan.target_pair[t]], results[(size_t)T + r], top, 0};
    }
    if (o.release)
        for (int i = 0; i < num_items; i++) (void)ferrum_hip_model_release(m, items[i].seq_id);
    return rc;
}

int ferrum_hip_model_decode_steps(FerrumHipModel* m, const uint64_t* seq_ids, const uint32_t* first_tokens, int n,
                                  int steps, uint32_t* out_tokens) {
    FH_REQUIRE(m && m->finalized && seq_ids && first_tokens, "decode_steps: bad argument");
    if (n <= 0 || steps <= 0) return 0;
    const FerrumHipModelConfig& c = m->cfg;
    FH_REQUIRE(n <= c.max_seqs && n <= 1024, "decode_steps: %d sequences > max_seqs %d (or 1024)", n, c.max_seqs);
    // admission for the whole run up front: block tables are then constant across the steps
    std::vector<FerrumHipKvSlotRequest> reqs(n);
    StepShape sh{};
    sh.m_total = sh.num_seqs = sh.num_sampled = n;
    sh.max_q_len = 1;
    // uniform sliding window: every layer takes the windowed varlen path (cu / pos live on the device like kv_lens);
    // a local/global pattern decides per layer inside enqueue_forward
    sh.pure_decode = !(c.sliding_window > 0 && c.sliding_window_pattern == 0);
    sh.all_single_token = true;
    for (int i = 0; i < n; i++) {
        const int len = m->seqs->len(seq_ids[i]);
        FH_REQUIRE(len > 0, "decode_steps: sequence %llu has no prefilled context", (unsigned long long)seq_ids[i]);
        FH_REQUIRE(len + steps <= c.max_seq_len, "decode_steps: sequence %llu would exceed max_seq_len", (unsigned long long)seq_ids[i]);
        FH_REQUIRE(first_tokens[i] < (uint32_t)c.vocab, "decode_steps: token out of vocab");
        reqs[i] = {seq_ids[i], len + steps, 0};
        sh.max_kv_len = std::max(sh.max_kv_len, len + steps);
    }
    if (int rc = m->seqs->reserve(reqs.data(), n, nullptr)) return rc;
    const size_t history_want = (size_t)std::max(steps * n, 4096) * 4;   // rarely regrown: 4096 ids cover 128 steps of 32 sequences
    if (m->history_bytes < history_want) {
        // the captured step holds the history pointer as a kernel argument: a graph recorded against the old buffer must
        // not be replayed (it would write the sampled ids into freed memory)
        drop_graph(m);
        if (int rc = grow_device((void**)&m->history, &m->history_bytes, history_want, m->stream)) return rc;
    }
    const IndexBlock h = index_block(m, m->idx_host);
    for (int i = 0; i < n; i++) {
        const SeqState& st = *m->seqs->find(seq_ids[i]);
        h.tokens[i] = first_tokens[i];
        h.cu[i] = (uint32_t)i;
        h.pos[i] = (uint32_t)st.len;
        h.kvl[i] = (uint32_t)st.len + 1;
        h.sampled_idx[i] = i;
        fill_block_table_row(m, h.bt + (size_t)i * m->max_blocks_per_seq, st);
    }
    h.cu[n] = (uint32_t)n;
    size_t used = m->il.block_tables + (size_t)n * m->max_blocks_per_seq * 4;
    FH_CHECK_HIP(hipMemcpyAsync(m->idx_dev, m->idx_host, used, hipMemcpyHostToDevice, m->stream));
    FH_CHECK_HIP(hipMemsetAsync(m->step_counter, 0, 8, m->stream));    // step index + the advance ticket

    auto enqueue_step = [&]() -> int {
        // the step's bookkeeping (sampled id → next input, positions, history) rides in the last stage of the argmax
        const IndexBlock d = index_block(m, m->idx_dev);
        DecodeAdvance adv;
        adv.tokens = d.tokens; adv.pos_offsets = d.pos; adv.kv_lens = d.kvl; adv.history = m->history; adv.step_counter = m->step_counter;
        adv.ticket = reinterpret_cast<unsigned*>(m->step_counter + 1); adv.n = n;
        int fused = 0;
        if (int rc = enqueue_forward(m, sh, true, nullptr, &adv, &fused)) return rc;
        if (!fused) {                                            // narrow vocabularies take the single-kernel argmax
            hipLaunchKernelGGL(decode_advance_kernel, dim3(1), dim3(1024), 0, m->stream, m->out_tokens, adv.tokens, adv.pos_offsets,
                               adv.kv_lens, m->history, m->step_counter, n);
            FH_CHECK_LAUNCH();
        }
        return 0;
    };

    // One decode step is captured into a hipGraph (BackendGraph, capabilities.rs:35-70) and
    // replayed: every per-step quantity lives in device buffers.  A graph is reusable while
    // (n, grid-shaping max_kv_len bucket) stay the same.
    // Tensor parallel: RCCL and the one-shot peer reduce are stream-ordered device work and are captured with the step;
    // only the host-barrier loopback of the tests cannot be.
    const bool use_graph = !(c.tp_world > 1 && m->tp_loopback) && !m->taps_enabled && !knobs().no_graph;
    int kv_bucket = cdiv(sh.max_kv_len, 256) * 256;
    sh.max_kv_len = kv_bucket;
    bool graph_ok = use_graph && !m->graph_refused;
    if (graph_ok && (!m->graph_exec || m->graph_n != n || m->graph_max_kv != kv_bucket)) {
        drop_graph(m);
        FH_CHECK_HIP(hipStreamSynchronize(m->stream));
        form_hit(FORM_GRAPH_CAPTURE);
        // (relaxed mode under tensor parallelism: the collective library may touch the allocator inside the capture window)
        FH_CHECK_HIP(hipStreamBeginCapture(m->stream, c.tp_world > 1 ? hipStreamCaptureModeRelaxed : hipStreamCaptureModeThreadLocal));
        int rc = enqueue_step();
        hipError_t e = hipStreamEndCapture(m->stream, &m->graph);
        if (!rc && e == hipSuccess) e = hipGraphInstantiate(&m->graph_exec, m->graph, nullptr, nullptr, 0);
        if (rc || e != hipSuccess) {
            // A step with a collective inside that the runtime will not capture (tensor parallel only): run it eagerly from now
            // on rather than fail — the capture attempt enqueued nothing, so the device state is untouched.
            (void)hipGetLastError();
            drop_graph(m);
            if (c.tp_world <= 1) {
                if (rc) return rc;
                FH_CHECK_HIP(e);
            }
            fprintf(stderr, "[ferrum_hip] decode step could not be captured under tensor parallelism (%s): eager launches from here on\n",
                    rc ? fh::last_error() : hipGetErrorString(e));
            m->graph_refused = true;
            graph_ok = false;
        } else {
            m->graph_n = n;
            m->graph_max_kv = kv_bucket;
        }
    }
    if (graph_ok) {
        for (int st = 0; st < steps; st++) { FH_CHECK_HIP(hipGraphLaunch(m->graph_exec, m->stream)); form_hit(FORM_GRAPH_REPLAY); }
    } else {
        for (int st = 0; st < steps; st++)
            if (int rc = enqueue_step()) return rc;
    }
    if (out_tokens)
        FH_CHECK_HIP(hipMemcpyAsync(out_tokens, m->history, (size_t)steps * n * 4, hipMemcpyDeviceToHost, m->stream));
    FH_CHECK_HIP(hipStreamSynchronize(m->stream));
    for (int i = 0; i < n; i++) m->seqs->advance(seq_ids[i], steps);
    return check_inlaunch_waits(m);
}

// Bench instrumentation: average device time of ONE launch of a hot kernel, measured with HIP events
// on the model's stream.  The launch is repeated over every layer's weights (L distinct weight sets,
// far larger than the 256 MiB Infinity Cache) using the routing / index state the last forward left
// in the scratch buffers, `reps` rounds.  which: 0 MoE gate_up (+silu·mul), 1 MoE down,
// 2 paged decode attention, 3 qkv GEMM, 4 o GEMM, 5 lm_head GEMM, 8 MoE gate_up → down as ONE launch.  Returns the mean microseconds per
// launch and (for MoE) the number of 16-row expert blocks the routing holds.
int ferrum_hip_model_time_kernel(FerrumHipModel* m, int which, int n_seqs, int max_kv_len, int reps, float* avg_us,
                                 int* moe_blocks) {
    FH_REQUIRE(m && m->finalized && avg_us && reps > 0, "time_kernel: bad argument");
    const FerrumHipModelConfig& c = m->cfg;
    hipStream_t s = m->stream;
    const int T = n_seqs, H = c.hidden;
    hipEvent_t e0, e1;
    FH_CHECK_HIP(hipEventCreate(&e0));
    FH_CHECK_HIP(hipEventCreate(&e1));
    int blocks = 0;
    const int P = T * std::max(c.top_k, 1), E = c.num_experts > 0 ? m->ep_E : 0;
    const int32_t* eids = moe_ids(m);
    if (E > 0 && (which < 2 || which == 8)) {
        FH_REQUIRE(P <= 1024, "time_kernel: MoE timing uses the decode (inline-align) path, pairs=%d > 1024", P);
        std::vector<int32_t> ids(P);
        FH_CHECK_HIP(hipMemcpyAsync(ids.data(), eids, (size_t)P * 4, hipMemcpyDeviceToHost, s));
        FH_CHECK_HIP(hipStreamSynchronize(s));
        std::vector<int> cnt(E, 0);
        for (int v : ids) if (v >= 0 && v < E) cnt[v]++;
        for (int e = 0; e < E; e++) blocks += (cnt[e] + 15) / 16;
    }
    if (moe_blocks) *moe_blocks = blocks;
    FH_REQUIRE(T <= c.max_tokens, "time_kernel: %d rows > max_tokens %d", T, c.max_tokens);
    const int max_blocks = E > 0 ? moe_max_blocks(P, E) : 0;
    int launches = 0, rc = 0;
    const bool em = E > 0 && moe_expert_major(m, P);
    auto one = [&](int li) -> int {
        LayerWeights& L = m->layers[li];
        switch (which) {
        case 0: {
            if (em) return w4_gemm_moe_expert_major(L.exp_gate_up, m->norm_out, m->moe_act, eids, E, P, c.top_k, 1, s);
            return w4_gemm_moe_inline_align(L.exp_gate_up, m->norm_out, m->moe_act, eids, E, P, max_blocks, c.top_k, 1,
                                            m->sorted_ids, m->block_ids, m->total_post_pad, s);
        }
        case 1:
            if (em) return w4_gemm_moe_expert_major(L.exp_down, m->moe_act, m->moe_down, eids, E, P, 1, 0, s);
            return w4_gemm_moe(L.exp_down, m->moe_act, m->moe_down, m->sorted_ids, m->block_ids, m->total_post_pad, P, max_blocks, 1, 0, s);
        case 8: {   // gate_up → down as the step runs them: one merged launch (falls back to an error when the shapes do not take it)
            unsigned *cur = arrive_half(m, launches & 1), *nxt = arrive_half(m, (launches & 1) ^ 1);
            int took = 0;
            // (as the step runs it: from the candidate lists the last chain launch left, where that is the layer's form)
            const MoeRouteLists lists = route_lists(m, T, chain_route_parts(m));
            const bool from_lists = lists.Q > 1 && knobs().decode_chain && moe_pair_rank_lists_ok(m, L, T, lists.Q);
            if (int r_ = w4_gemm_moe_expert_major_pair(L.exp_gate_up, L.exp_down, m->norm_out, m->moe_act, m->moe_down, eids, E, P, c.top_k,
                                                       cur, nxt, m->inlaunch_timeouts, &took, s, from_lists ? &lists : nullptr)) return r_;
            if (!took) { fh::set_error("time_kernel: the merged gate_up → down launch does not take these shapes"); return FERRUM_HIP_UNSUPPORTED; }
            return 0;
        }
        case 2: return paged_batched_decode_attention_f16(m->q_out, L.k_pool, L.v_pool, m->attn_out, index_block(m, m->idx_dev).bt,
                                                          index_block(m, m->idx_dev).kvl, T, max_kv_len, c.num_heads, c.num_kv_heads,
                                                          c.head_dim, KV_BLOCK, m->max_blocks_per_seq, m->workspace, m->workspace_bytes, s);
        case 3: return w4_gemm_dense(L.qkv, m->norm_out, m->qkv_out, T, m->workspace, m->workspace_bytes, s);
        case 4: return w4_gemm_dense(L.o, m->attn_out, m->o_out, T, m->workspace, m->workspace_bytes, s);
        case 6: return w4_gemm_dense(L.gate_up, m->norm_out, m->gate_up_out, T, m->workspace, m->workspace_bytes, s);
        case 7: return w4_gemm_dense(L.down, m->act_out, m->mlp_out, T, m->workspace, m->workspace_bytes, s);
        case 5: return f16t_gemm_f32out(m->sampled_hidden, m->lm_head_t, m->logits, T, m->vp_n, H, m->workspace, m->workspace_bytes, s);
        }
        fh::set_error("time_kernel: which=%d", which);
        return FERRUM_HIP_INVALID;
    };
    FH_REQUIRE((which >= 2 && which != 8) || E > 0, "time_kernel: MoE kernel on a dense model");
    FH_REQUIRE(which < 6 || which == 8 || E == 0, "time_kernel: dense MLP kernel on a MoE model");
    if (which == 8) {
        FH_REQUIRE(em && knobs().moe_em2 && m->em2_arrive && !m->em2_failed, "time_kernel: the merged gate_up → down launch is not what this batch takes");
        FH_CHECK_HIP(hipMemsetAsync(m->em2_arrive, 0, 2 * m->arrive_half_words * sizeof(unsigned), s));
    }
    const bool same_layer = knobs().time_same_layer;   // experiment: weights resident in the Infinity Cache
    // warm-up round (code objects, TLBs), then the timed rounds
    for (int li = 0; li < c.num_layers && !rc; li++) { rc = one(li); if (which == 8) launches++; }
    if (which == 8 && (launches & 1)) { rc = rc ? rc : one(0); launches++; }      // (even count: the counter halves alternate)
    launches = 0;
    if (rc) return rc;
    FH_CHECK_HIP(hipEventRecord(e0, s));
    for (int r = 0; r < reps && !rc; r++)
        for (int li = 0; li < c.num_layers && !rc; li++) { rc = one(which == 5 || same_layer ? 0 : li); launches++; }
    FH_CHECK_HIP(hipEventRecord(e1, s));
    FH_CHECK_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    FH_CHECK_HIP(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc) return rc;
    *avg_us = ms * 1000.0f / (float)launches;
    return 0;
}

}  // extern "C"
