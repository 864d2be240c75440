// Host-side launchers for the HIP/CDNA4 kernels (raw pointers + hipStream_t, so the
// torch binding translation unit does not need the device compiler's headers).
#pragma once

#include <hip/hip_runtime_api.h>
#include <stdint.h>

constexpr int kActSwiglu = 4;  // == ACT_SWIGLU in common.h (device-side enum)

// RoPE applied in a GEMM epilogue to output columns [0, cols): the q/k rows of the weight are
// PAIR-INTERLEAVED per head (column 2i <-> d_i, 2i+1 <-> d_{i+D/2}), so a rotary pair is two
// adjacent columns of one lane; position = row % S; cos/sin tables are fp32 [S][D/2].
struct RopeArgs {
  const float* cos = nullptr;
  const float* sin = nullptr;
  int S = 1, D = 2, cols = 0;  // cols == 0: off
};

struct GemmArgs {
  const void* A;  // bf16 [M][lda]
  int lda;
  const void* W;  // bf16 [N][ldw]
  int ldw;
  void* C;        // bf16 [M][ldc]
  int ldc;
  const void* bias;  // bf16 [N] or nullptr
  const void* R;     // bf16 [M][ldr] residual or nullptr
  int ldr;
  int M, N, K;
  int act;       // DlsAct
  float alpha;
  int config;    // -1 = auto
  int compact_rows = 0;  // > 0 with a device row range [r0, r1): write output rows 0..r1-r0-1 (not r0..),
                         // and at most compact_rows of them (the output's row capacity)
  // grouped launches whose groups share weights (a cross-request expert batch: one group per
  // (request, expert)): the groups of one weight panel run on consecutive workgroups of one XCD
  // and the weights keep the default cache policy, so each panel comes from HBM once
  int grouped_shared = 0;
  RopeArgs rope{};
  // Row statistics hand-off between a residual-producing GEMM and the next folded norm:
  // stats_out: fp32 [M][2] (zeroed by the caller) += (sum, sum of squares) of each FINAL
  //            (bf16-rounded) output row — the producer's epilogue emits them for free;
  // ext_stats: read them instead of accumulating them in the consumer's main loop (with
  //            ln_mode 1/2 and ln_colsum: any tile config, split-K allowed).
  float* stats_out = nullptr;
  const float* ext_stats = nullptr;
  // split-K: >= tiles_m*tiles_n zeroed counters, in tiles of the config the launch resolves to
  // (gemm_glds_resolve, gemm_glds_tile) -> combine inside the GEMM launch
  int* tile_sem = nullptr;
  // post-norm of the FINAL output rows for the next (unfolded) norm: norm_out[M][ldn] =
  // norm(C) * norm_w (+ norm_b); norm_mode 1 LayerNorm, 2 RMSNorm. Split-K launches do it in
  // their row-owning reduce (no separate norm launch); launch_gemm_glds reports whether it did.
  void* norm_out = nullptr;
  const void* norm_w = nullptr;
  const void* norm_b = nullptr;
  int norm_mode = 0;
  float norm_eps = 1e-5f;
  int ldn = 0;
  // cache policy of a plain split-ring launch (LN 0): bit 0 the weight DMA streams (nt), bit 1
  // the output stores stream (nt) — for a weight read once per step and a write-once output
  // (the LM head's 77 MB weight and 51 MB of logits) that should not displace the layer
  // weights from the Infinity Cache
  int stream_pol = 0;
};

// epilogue extras carried down to the tile code
struct Epi {
  RopeArgs rope;
  float* stats_out;
  const float* ext_stats;
  // in-launch split-K combine: one arrival counter per output tile (zero before the launch,
  // reset by each tile's last arriver); nullptr -> separate reduce kernel
  int* tile_sem = nullptr;
  // grouped launch (every expert of an MoE layer in ONE grid): per-group weight pointers and,
  // for compact outputs, per-group output pointers (device arrays of E addresses)
  const unsigned long long* grp_w = nullptr;
  const unsigned long long* grp_c = nullptr;
  // grouped launch: weight DMA with the streaming (nt) cache policy (split-ring configs)
  int w_stream = 0;
};

int gemm_pick_config(int M, int N, int K);
void launch_gemm_bf16(const GemmArgs& a, hipStream_t s);  // register-staged, any K % 8 == 0

// LDS-DMA multistage GEMM (K % 64 == 0); split-K partials need workspace_bytes of fp32
int gemm_glds_num_configs();
int gemm_glds_kstep(int cfg);  // K granularity of a config (64, or 128 for two K groups)
void gemm_glds_tile(int cfg, int* bm, int* bn);  // output tile of a config (persistent flag ignored)
// the config launch_gemm_glds runs for (cfg, activation, folded norm with in-kernel statistics)
int gemm_glds_resolve(int cfg, int act, bool ln_in);
// cfg | kGemmPersist: the same tile config as a persistent launch (a resident grid walks the
// tiles; one tile's store drain overlaps the next tile's first loads)
constexpr int kGemmPersist = 64;
void gemm_glds_pick(int M, int N, int K, int* cfg, int* splitk);
size_t gemm_glds_workspace_bytes(int M, int N, int splitk);
// ln_mode: 0 none, 1 LayerNorm, 2 RMSNorm folded into the GEMM (A = raw input rows,
// W pre-scaled by the norm gain, ln_colsum[n] = sum_k W[n][k], bias = bias + W.ln_bias)
// rows (device int32[2], optional): only rows [rows[0], rows[1]) of A/C/R take part (M is then
// the maximum row count, sizing the grid) — an MoE expert's routed rows without a host sync.
// returns true when the launch also wrote a.norm_out (a split-K GEMM's row-owning reduce)
bool launch_gemm_glds(const GemmArgs& a, int cfg, int splitk, void* workspace, hipStream_t s,
                      const float* ln_colsum = nullptr, int ln_mode = 0, float ln_eps = 1e-5f,
                      const int* rows = nullptr);
// Wave-private rings (gemm_private.hip; gemm_glds_impl.h: mainloop_private): a family of its own
// for the skinny 32 x 48 tiles, ids kGemmPrivate + {0, 1, 2, 3} = W waves x S ring slots of
// 8 x 2, 4 x 3, 6 x 2, 12 x 1. It takes plain launches only — the whole K in one block with
// K % (64 W) == 0, no activation, folded norm, RoPE, SwiGLU, split-K or row range; bias, residual,
// stats_out and alpha are what it attaches (gemm_private_takes; the launcher launches nothing and
// returns false otherwise).
constexpr int kGemmPrivate = 120, kGemmPrivateCount = 4;
int gemm_private_waves(int cfg);  // W of a family id, 0 for any other id
bool gemm_private_takes(const GemmArgs& a, int cfg, int splitk, bool folded_norm, bool ranged);
bool launch_gemm_private(const GemmArgs& a, int cfg, hipStream_t s);
// The same rings on 64-row tiles with the folded-norm finish (gemm_private_wide_kernel), ids
// kGemmPrivateWide + i: one tile per CU at GPT-2's fc1 (512 x 3072 on 64 x 96) and QKV (512 x 2304
// on 64 x 80). It takes folded-norm launches whose row statistics come from ext_stats — the whole
// K in one block with K % (64 W) == 0, bias, no activation or GeLU; no RoPE, SwiGLU, split-K, row
// range, residual or stats_out (gemm_private_wide_takes; the launcher launches nothing and returns
// false otherwise).
constexpr int kGemmPrivateWide = 130, kGemmPrivateWideCount = 4;
struct GemmPrivateWideCfg {
  int bm, bn, waves, slots;  // tile, W waves x S ring slots
};
constexpr GemmPrivateWideCfg kGemmPrivateWideCfgs[kGemmPrivateWideCount] = {{64, 96, 4, 2}, {64, 96, 3, 2}, {64, 80, 4, 2}, {64, 80, 3, 2}};
int gemm_private_wide_waves(int cfg);  // W of a family id, 0 for any other id
bool gemm_private_wide_takes(const GemmArgs& a, int cfg, int splitk, int ln_mode, bool ranged);
bool launch_gemm_private_wide(const GemmArgs& a, int cfg, const float* ln_colsum, int ln_mode, float ln_eps,
                              hipStream_t s);

// Grouped MoE-expert GEMM: E groups in ONE launch (grid = E x column tiles). Group g multiplies
// rows [offsets[g], offsets[g+1]) of A by its own weight (w_ptrs[g], [N][K], ldw = a.ldw) and
// writes them either at the same rows of a.C (c_ptrs == nullptr) or compactly to rows
// 0..min(count, a.compact_rows)-1 of c_ptrs[g]. No split-K; any LDS-DMA config.
void launch_gemm_glds_grouped(const GemmArgs& a, int cfg, int n_groups, const int* offsets,
                              const unsigned long long* w_ptrs, const unsigned long long* c_ptrs, hipStream_t s,
                              const int* a_rows = nullptr);

// Grouped skinny GEMM (gemm_grouped_skinny.hip): the contract of launch_gemm_glds_grouped for
// bf16 without bias or residual and act in {ACT_NONE, ACT_SWIGLU}, for the <= 16 rows per group
// of a decode step: weights streamed straight to VGPRs, a workgroup per (group, 16-column strip),
// its waves split K and sum in a fixed order. Any counts (zero: no weight byte is requested;
// more than 16: further passes over the same weights). K % 32 == 0, N % 16 == 0 (SwiGLU:
// N % 32 == 0, N/2 outputs). The grid depends on (n_groups, N) only. No atomics, no host sync.
struct GemmGroupedSkinnyArgs {
  const void* A;  // bf16 [a_total][lda], lda % 8 == 0, 16-byte aligned
  int lda;
  int a_total;         // rows of A (a_rows values are clamped into it)
  const int* a_rows;   // device int32 [R] or nullptr
  const int* offsets;  // device int32 [n_groups + 1]
  const unsigned long long* w_ptrs;  // device [n_groups]: bf16 [N][K], 16-byte aligned
  const unsigned long long* c_ptrs;  // device [n_groups] or nullptr
  void* C;                           // bf16 [R][ldc] when c_ptrs == nullptr
  int ldc;
  int compact_rows;
  int R, N, K;  // R: rows all groups cover together (offsets are clamped to it)
  int act;
  int n_groups;
};
bool gemm_grouped_skinny_takes(int N, int K, int act);
void launch_gemm_grouped_skinny(const GemmGroupedSkinnyArgs& a, hipStream_t s);

// Dense skinny GEMM (gemm_skinny.hip): C = epi(alpha * A W^T) for the 1 <= M <= 16 rows of a decode
// step, bf16, weights streamed straight to VGPRs: a workgroup per 16-column strip of the output
// (SwiGLU: per 16-gate + 16-up block pair), its `waves` waves split K and sum in a fixed order. No
// atomics, no split-K across workgroups, no workspace. Any N (SwiGLU: N % 32 == 0), K % 32 == 0,
// lda % 8 == 0, ldw % 8 == 0, A and W 16-byte aligned. With ln_mode 1 (LayerNorm) / 2 (RMSNorm) A
// holds the raw rows, W / bias / ln_colsum the derived operands of a folded norm, and the kernel
// takes the row statistics itself. Row ranges, compact outputs, stats_out, ext_stats and
// post-norms are not part of the contract.
constexpr int kSkinnyMaxRows = 16;
struct GemmSkinnyArgs {
  const void* A;  // bf16 [M][lda]
  int lda;
  const void* W;  // bf16 [N][ldw]
  int ldw;
  void* C;  // bf16 [M][ldc] (SwiGLU: N/2 columns)
  int ldc;
  const void* bias;  // bf16 [N] or nullptr
  const void* R;     // bf16 [M][ldr] or nullptr
  int ldr;
  int M, N, K;
  int act;  // DlsAct
  float alpha;
  RopeArgs rope{};
  const float* ln_colsum = nullptr;  // fp32 [N]
  int ln_mode = 0;
  float ln_eps = 1e-5f;
  int stream = 0;  // weight loads: 1 streaming (nt), 0 default cache policy
  int waves = 0;   // 4, 8, 16; 0: gemm_skinny_waves
};
// false with *why (optional) naming the rule a launch breaks
bool gemm_skinny_takes(const GemmSkinnyArgs& a, const char** why = nullptr);
int gemm_skinny_waves(int N, int K, int act);  // waves per workgroup the launcher picks: 4, 8 or 16
bool launch_gemm_skinny(const GemmSkinnyArgs& a, hipStream_t s);  // false: nothing launched

// W8A16 GEMM (gemm_w8.hip): C = act(alpha * scale[n] * sum_k A[m][k] * Wq[n][k] + bias[n]) + R
// with Wq stored as OCP e4m3 bytes ([N][ldw], K contiguous) and one fp32 scale per output
// channel. The fp8 bytes go through LDS, are converted to bf16 in registers (exact) and run on
// the bf16 MFMA; the scale is applied in the epilogue. K % 16 == 0, any M, N (even for SwiGLU).
struct GemmW8Args {
  const void* A;  // bf16 [M][lda]
  int lda;
  const void* Wq;  // e4m3 [N][ldw]
  int ldw;
  const float* scale;  // fp32 [N], positive
  void* C;             // bf16 [M][ldc] (SwiGLU: N/2 columns)
  int ldc;
  const void* bias;  // bf16 [N] or nullptr
  const void* R;     // bf16 [M][ldr] or nullptr
  int ldr;
  int M, N, K;
  int act;  // DlsAct
  float alpha;
  int config;       // 0..gemm_w8_num_configs()-1
  int splitk;       // >= 1; > 1: fp32 partial slabs in `workspace`, summed in a fixed order
  float* workspace;  // gemm_w8_workspace_bytes() when splitk > 1
  int store_pol;     // output stores: 0 plain, 2 nt, 4 write-through (GemmArgs::stream_pol bits 1, 2)
};
int gemm_w8_num_configs();
void gemm_w8_pick(int M, int N, int K, int* cfg, int* splitk);
// the largest split of K a config takes for this K (every split covers whole K tiles)
int gemm_w8_max_splitk(int cfg, int K);
size_t gemm_w8_workspace_bytes(int M, int N, int splitk);
void launch_gemm_w8(const GemmW8Args& a, hipStream_t s);

// Grouped W8A16 GEMM (gemm_w8_grouped.hip): the contract of launch_gemm_glds_grouped with the
// arithmetic of launch_gemm_w8. n_groups groups in ONE launch; group g multiplies rows
// [offsets[g], offsets[g+1]) — row r of A, or token row a_rows[r] of A — by its e4m3 weight
// w_ptrs[g] ([N][K], K contiguous) with channel scales s_ptrs[g] (fp32 [N]) and writes them at
// the same rows of C (c_ptrs == nullptr) or compactly to rows 0..min(count, compact_rows)-1 of
// c_ptrs[g] ([.][ldc]). act: ACT_NONE or ACT_SWIGLU (rows and scales interleaved in blocks of
// 16, N/2 outputs, N % 32 == 0). K % 16 == 0, any N, any counts (zero included). No split-K,
// no atomics, no host sync.
struct GemmW8GroupedArgs {
  const void* A;  // bf16 [.][lda]
  int lda;
  const int* a_rows;  // device int32 [R] or nullptr
  const int* offsets;  // device int32 [n_groups + 1]
  const unsigned long long* w_ptrs;  // device [n_groups]
  const unsigned long long* s_ptrs;  // device [n_groups]
  const unsigned long long* c_ptrs;  // device [n_groups] or nullptr
  void* C;                           // bf16 [R][ldc] when c_ptrs == nullptr
  int ldc;
  int compact_rows;
  int R, N, K;  // R: rows all groups cover together (offsets are clamped to it)
  int act;
  int n_groups;
  int config;          // 0..gemm_w8_grouped_num_configs()-1
  int shared_weights;  // groups repeat weights, same-weight groups adjacent: they run side by side
  int store_pol;       // as GemmW8Args::store_pol
};
int gemm_w8_grouped_num_configs();
int gemm_w8_grouped_tile_rows(int cfg);  // row-tile height of a config
int gemm_w8_grouped_pick(int rows_hint, int N, int K, int n_groups);
void launch_gemm_w8_grouped(const GemmW8GroupedArgs& a, hipStream_t s);

// W8A8 GEMM (gemm_w8a8.hip): C = act(alpha * xscale[m] * scale[n] * sum_k Aq[m][k] * Wq[n][k] +
// bias[n]) + R with BOTH operands OCP e4m3 bytes (K contiguous), one fp32 scale per activation
// row and one per output channel, on the block-scaled fp8 MFMA (16x16x128, neutral block
// scales); the two scales are applied in the epilogue. K % 16 == 0, any M, N (even for SwiGLU).
struct GemmW8A8Args {
  const void* Aq;  // e4m3 [M][lda]
  int lda;
  const float* xscale;  // fp32 [M], positive
  const void* Wq;       // e4m3 [N][ldw]
  int ldw;
  const float* scale;  // fp32 [N], positive
  void* C;             // bf16 [M][ldc] (SwiGLU: N/2 columns)
  int ldc;
  const void* bias;  // bf16 [N] or nullptr
  const void* R;     // bf16 [M][ldr] or nullptr
  int ldr;
  int M, N, K;
  int act;  // DlsAct
  float alpha;
  int config;        // 0..gemm_w8a8_num_configs()-1
  int splitk;        // >= 1; > 1: fp32 partial slabs in `workspace`, summed in a fixed order
  float* workspace;  // gemm_w8a8_workspace_bytes() when splitk > 1
  int store_pol;     // as GemmW8Args::store_pol
};
int gemm_w8a8_num_configs();
void gemm_w8a8_pick(int M, int N, int K, int* cfg, int* splitk);
int gemm_w8a8_max_splitk(int cfg, int K);
size_t gemm_w8a8_workspace_bytes(int M, int N, int splitk);
void launch_gemm_w8a8(const GemmW8A8Args& a, hipStream_t s);

// W4A8 GEMM (gemm_w4a8.hip): C = act(alpha * xscale[m] * sum_k Aq[m][k] * W[n][k] + bias[n]) + R
// with e4m3 activation rows (one fp32 scale per row) and OCP MXFP4 weights: Wq [N][K/2] bytes, two
// e2m1 per byte (even k in the low nibble), Ws [N][K/32] e8m0 block scales, on the block-scaled
// MFMA (16x16x128, fp4 x fp8). K % 32 == 0, any M, N (N % 32 == 0 for SwiGLU).
struct GemmW4A8Args {
  const void* Aq;  // e4m3 [M][lda]
  int lda;
  const float* xscale;  // fp32 [M], positive
  const void* Wq;       // e2m1 pairs [N][ldw bytes]
  int ldw;
  const void* Ws;  // e8m0 [N][lds], codes 0..254
  int lds;
  void* C;  // bf16 [M][ldc] (SwiGLU: N/2 columns)
  int ldc;
  const void* bias;  // bf16 [N] or nullptr
  const void* R;     // bf16 [M][ldr] or nullptr
  int ldr;
  int M, N, K;
  int act;  // DlsAct
  float alpha;
  int config;        // 0..gemm_w4a8_num_configs()-1
  int splitk;        // >= 1; > 1: fp32 partial slabs in `workspace`, summed in a fixed order
  float* workspace;  // gemm_w4a8_workspace_bytes() when splitk > 1
  int store_pol;     // as GemmW8Args::store_pol
};
int gemm_w4a8_num_configs();
void gemm_w4a8_pick(int M, int N, int K, int* cfg, int* splitk);
int gemm_w4a8_max_splitk(int cfg, int K);
size_t gemm_w4a8_workspace_bytes(int M, int N, int splitk);
void launch_gemm_w4a8(const GemmW4A8Args& a, hipStream_t s);

// Grouped W4A8 GEMM (gemm_w4a8_grouped.hip): the contract of launch_gemm_w8_grouped with the
// arithmetic of launch_gemm_w4a8. Group g multiplies the sorted rows [offsets[g], offsets[g+1]) —
// row r of Aq, or token row a_rows[r] — by its MXFP4 weight: e2m1 pairs [N][K/2] at w_ptrs[g],
// e8m0 block scales [N][K/32] at s_ptrs[g] (codes 0..254). xscale holds one fp32 scale per SOURCE
// row of Aq: sorted row r takes xscale[a_rows[r]]. act: ACT_NONE or ACT_SWIGLU (rows of q and s
// interleaved in blocks of 16, N % 32 == 0). K % 32 == 0, any N, any counts (zero included). No
// split-K, no atomics, no host sync.
struct GemmW4A8GroupedArgs {
  const void* Aq;  // e4m3 [.][lda bytes], rows 16-byte aligned
  int lda;
  const float* xscale;  // fp32, one per row of Aq
  const int* a_rows;    // device int32 [R] or nullptr
  const int* offsets;   // device int32 [n_groups + 1]
  const unsigned long long* w_ptrs;  // device [n_groups]
  const unsigned long long* s_ptrs;  // device [n_groups]
  const unsigned long long* c_ptrs;  // device [n_groups] or nullptr
  void* C;                           // bf16 [R][ldc] when c_ptrs == nullptr
  int ldc;
  int compact_rows;
  int R, N, K;  // R: rows all groups cover together (offsets are clamped to it)
  int act;
  int n_groups;
  int config;           // 0..gemm_w4a8_grouped_num_configs()-1
  int shared_weights;   // as GemmW8GroupedArgs::shared_weights
  int store_pol;        // as GemmW8Args::store_pol
  int scales_aligned4;  // every scale tensor's base is 4-byte aligned (with K % 128 == 0: dword loads)
};
int gemm_w4a8_grouped_num_configs();
int gemm_w4a8_grouped_tile_rows(int cfg);  // row-tile height of a config
int gemm_w4a8_grouped_pick(int rows_hint, int N, int K, int n_groups);
void launch_gemm_w4a8_grouped(const GemmW4A8GroupedArgs& a, hipStream_t s);

// Per-row e4m3 quantisation (quant_rows.hip): q[m][k] = rne(x[m][k] / scale[m]) with scale[m] the
// smallest power of two with amax_m / scale[m] <= 448 (all-zero row: 1). x bf16 [M][ldx],
// q e4m3 [M][ldq], K % 8 == 0.
void launch_quant_rows_fp8(const void* x, int ldx, void* q, int ldq, float* scale, int M, int K, hipStream_t s);
// launch_layernorm / launch_rmsnorm emitting the quantised rows of their (bf16-rounded) output:
// q e4m3 [M][H] contiguous, scale fp32 [M]
void launch_layernorm_q8(const void* x, const void* r, void* sum_out, const void* w, const void* b, void* q,
                         float* scale, int M, int H, float eps, hipStream_t s);
void launch_rmsnorm_q8(const void* x, const void* r, void* sum_out, const void* w, void* q, float* scale, int M,
                       int H, float eps, hipStream_t s);

struct AttnArgs {
  const void* q; int ldq;   // bf16, row = token (b*S + s), head h at column h*D
  const void* k; int ldk;   // kv head g at column g*D
  const void* v; int ldv;
  void* o; int ldo;         // bf16 output, head h at column h*D
  int B, S, n_head, n_kv_head, D;
  float scale;
  int causal;
  int variant = 0;  // 0 auto; 1..11 fixed (waves, K/V stages, key split) — benchmarks/tuning
  // Sequence-chunked attention (context parallelism as a DAG): q holds Sq query rows per
  // batch at global positions q_off .. q_off+Sq-1; k/v hold S key rows per batch (positions
  // 0 .. S-1). Sq = 0 means Sq = S, q_off = 0 (ordinary self-attention).
  int Sq = 0;
  int q_off = 0;
  int flags = 0;  // bit 0: output stores write-through (sc1); bit 1: XCD-grouped blocks
  void* part = nullptr;  // variant 14: fp32 partials, attention_split_sizes() floats
  void* cnt = nullptr;   // variant 14: int32 tickets, zero before the first launch (self-resetting)
};
void launch_attention_fwd(const AttnArgs& a, hipStream_t s);
void attention_split_sizes(const AttnArgs& a, size_t* part_floats, size_t* counters);

// KV cache and decode steps (attn_decode.hip, attn_decode_fp8.hip). The caches are bf16
// [B][C][n_kv_head*D], or with kv_fp8 e4m3 bytes of that shape plus fp32 power-of-two scales
// [B][n_kv_head][C], one per (position, KV head); pos is int32 [B] in device memory (the length of
// every sequence before the step), so one captured launch serves every step.
struct DecodeArgs {
  const void* q; int ldq;  // bf16 [B*T][>= n_head*D], row b*T + t, head h at column h*D
  const void* k_cache;     // bf16 [B][C][n_kv_head*D]; kv_fp8: e4m3 bytes
  const void* v_cache;
  void* o; int ldo;        // bf16 [B*T][>= n_head*D]
  const int* pos;          // int32 [B]: query t of sequence b sits at position pos[b] + t
  int B, T, C, n_head, n_kv_head, D;
  float scale;
  int chunk = 0;           // keys per workgroup (a multiple of 64); 0: attn_decode_chunk()
  void* part = nullptr;    // fp32 partials, attn_decode_sizes() floats
  void* cnt = nullptr;     // int32 tickets, zero before the first launch (self-resetting)
  bool kv_fp8 = false;     // e4m3 caches with the two scale tensors below
  const float* k_scale = nullptr;  // fp32 [B][n_kv_head][C]
  const float* v_scale = nullptr;
};
// T in 1..16, (n_head / n_kv_head) * T <= 64, D 64 or 128
bool attn_decode_supported(int T, int n_head, int n_kv_head, int D);
// the launcher's keys per workgroup: the grid (ceil(C / chunk), n_kv_head, B) fills 256 CUs where C allows
int attn_decode_chunk(int B, int C, int n_kv_head, int D);
void attn_decode_sizes(const DecodeArgs& a, size_t* part_floats, size_t* counters);
void launch_attn_decode(const DecodeArgs& a, hipStream_t s);
void launch_attn_decode_fp8(const DecodeArgs& a, hipStream_t s);  // what launch_attn_decode calls with kv_fp8
// rows pos[b] .. pos[b]+T-1 of sequence b's caches = rows b*T .. b*T+T-1 of k_new / v_new
// (bf16 [B*T][>= n_kv_head*D] views, 16-byte aligned rows); rows at or past C are dropped.
// With k_scale / v_scale (fp32 [B][n_kv_head][C]) the caches are e4m3 bytes: every head's D values
// of a row are quantised by the rule of quantize_fp8 and the scale lands at [b][h][pos[b]+t]
// (row_elems / n_kv_head a multiple of 8, at most 128).
void launch_kv_append(const void* k_new, int ldk, const void* v_new, int ldv, void* k_cache, void* v_cache,
                      float* k_scale, float* v_scale, const int* pos, int B, int T, int C, int row_elems,
                      int n_kv_head, hipStream_t s);
void launch_kv_append_fp8(const void* k_new, int ldk, const void* v_new, int ldv, void* k_cache, void* v_cache,
                          float* k_scale, float* v_scale, const int* pos, int B, int T, int C, int n_kv_head, int D,
                          hipStream_t s);
// tok_out[b*T + t] = tokens[b][p], out_i[b*T + t] = tab_i[p] (rows of row_bytes_i, a multiple of 16;
// tab_i may be null) with p = min(pos[b] + t, C - 1)
void launch_decode_prologue(const int* pos, const int* tokens, int* tok_out, const void* tab0, void* out0,
                            int row_bytes0, const void* tab1, void* out1, int row_bytes1, int B, int T, int C,
                            hipStream_t s);

// Chunk attention over the cache (attn_chunk.hip): T queries per sequence, 1 <= T <= 1024, query
// row b*T + t against cache rows 0 .. min(pos[b]+t, C-1) of sequence b; rows at or past pos[b]+T
// are never read. bf16 caches only (fp8 ones go through launch_kv_dequantize_rows first).
struct ChunkAttnArgs {
  const void* q; int ldq;  // bf16 [B*T][>= n_head*D]
  const void* k_cache;     // bf16 [B][C][n_kv_head*D]
  const void* v_cache;
  void* o; int ldo;        // bf16 [B*T][>= n_head*D]
  const int* pos;          // int32 [B], read by the kernel
  int B, T, C, n_head, n_kv_head, D;
  float scale;
  int variant = 0;         // 0: by block count; 2, 8, 13: that configuration of attention.hip
};
bool attn_chunk_supported(int T, int n_head, int n_kv_head, int D);
int attn_chunk_variant(int B, int T, int n_head, int variant);  // the configuration a launch takes
void launch_attn_chunk(const ChunkAttnArgs& a, hipStream_t s);
// out[b][r] = e4m3 cache[b][r] x scale[b][h][r] as bf16 for r < min(pos[b]+T, C); no other row is written
void launch_kv_dequantize_rows(const void* cache, const float* scale, const int* pos, void* out, int B, int T, int C,
                               int n_kv_head, int D, hipStream_t s);
// pos[b] = min(pos[b] + T, max(limit[b], pos[b]))
void launch_kv_advance(int* pos, const int* limit, int B, int T, hipStream_t s);

// Token sampling over the last logits row of every sequence (sample.hip): greedy, temperature,
// top-k and top-p by whole value classes, a Philox4x32-10 draw in index order, and the stream
// rule that feeds the token back into tokens[b][pos[b]+T]. One launch; a row is split over
// `slices` workgroups whose partials the last arriver merges.
struct SampleArgs {
  const void* logits; int ld;  // bf16 [B*T][ld]; row b*T + T-1 is read, V valid columns
  int V, B, T, C;
  const int* pos;              // [B] sequence lengths before the step (never written)
  int* tokens;                 // [B][C] token stream
  const float* temperature;    // [B], 0 = greedy
  const int* top_k;            // [B], 0 = off
  const float* top_p;          // [B], >= 1 = off
  const long long* seed;       // [1]
  int request;                 // replica ordinal: Philox counter word 2
  const int* prompt_len;       // [B] or null (0)
  const int* eos;              // [1] or null (-1)
  int* done;                   // [B] or null
  int* next_out;               // [B]
  float* stats;                // [B][4]: theta, Z, cumulative weight before the token, its weight
  unsigned* part;              // sample_sizes() words, written and read inside the launch
  int* cnt;                    // [B] tickets: zero before the first launch, reset by the launch
};
constexpr int kSampleMaxV = 1 << 20;
// workgroups per row and elements per workgroup (a multiple of 8) for B rows of V logits
void sample_slices(int B, int V, int* slices, int* slice_len);
void sample_sizes(int B, int V, size_t* part_words, size_t* counters);
void launch_sample(const SampleArgs& a, hipStream_t s);

// y = LN(x [+ r]) * w + b ; if r != nullptr and sum_out != nullptr, sum_out = x + r
void launch_layernorm(const void* x, const void* r, void* sum_out, const void* w, const void* b, void* y, int M,
                      int H, float eps, hipStream_t s);
void launch_rmsnorm(const void* x, const void* r, void* sum_out, const void* w, void* y, int M, int H, float eps,
                    hipStream_t s);

void launch_gelu(const void* x, void* y, int64_t n, hipStream_t s);
void launch_add(const void* a, const void* b, void* y, int64_t n, hipStream_t s);
void launch_swiglu(const void* gu, void* y, int M, int F, hipStream_t s);  // gu [M][2F] (gate|up)
void launch_embedding(const int32_t* tokens, const void* wte, const void* wpe, void* y, int M, int S, int H,
                      hipStream_t s, float* zbuf = nullptr, int zn = 0, float* stats = nullptr);
// in-place rotary embedding on the q and k head slices of a packed qkv row buffer
void launch_rope(void* qkv, int ld, int M, int S, int n_head, int n_kv_head, int D, int k_col, const float* cos_t,
                 const float* sin_t, hipStream_t s);

// MoE
void launch_moe_router(const void* logits, int M, int E, int topk, int32_t* topk_idx, float* topk_w,
                       hipStream_t s);
void launch_moe_align(const int32_t* topk_idx, int M, int topk, int E, int32_t* src_rows, int32_t* slot_of,
                      int32_t* offsets, hipStream_t s);
// router + align in one workgroup (M * topk <= kRouteMaxAssign): same outputs as the pair
constexpr int kRouteMaxAssign = 16384;
void launch_moe_route(const void* logits, int M, int E, int topk, int32_t* topk_idx, float* topk_w,
                      int32_t* src_rows, int32_t* slot_of, int32_t* offsets, hipStream_t s);
// router GEMM (logits = x Wg^T, bf16) + routing in one launch; false (nothing launched) when
// the shape is outside its limits (E * H <= 32768, M * max(k, E) <= kRouteMaxAssign, E even, E <= 16)
bool launch_moe_gate_route(const void* x, int ldx, const void* wg, int M, int H, int E, int topk, void* logits,
                           int* ticket, int32_t* topk_idx, float* topk_w, int32_t* src_rows, int32_t* slot_of,
                           int32_t* offsets, hipStream_t s);
void launch_moe_permute(const void* x, const int32_t* src_rows, void* out, int rows, int H, hipStream_t s);
// cross-request expert batch: per group g = (request req[g], expert expert[g]) the device-side
// row range of that request's routing (off[req]: int32 [E+1]) placed at base[req] — writes the
// groups' offsets [G+1] and the token row of every sorted row (a_rows) for one grouped launch
constexpr int kXbatchMaxReq = 16, kXbatchMaxGroups = 64;
struct XbatchIndexArgs {
  const int32_t* off[kXbatchMaxReq];
  int32_t base[kXbatchMaxReq];
  int32_t req[kXbatchMaxGroups];
  int32_t expert[kXbatchMaxGroups];
  int G;
  int32_t* offsets;
  int32_t* a_rows;
};
void launch_moe_xbatch_index(const XbatchIndexArgs& a, hipStream_t s);
// Expert-parallel capacity edges (fixed-size RCCL messages, parallel/executor.py): the rows a
// layer's routing sends to one expert GPU, packed (home rank) into / unpacked (expert GPU) from
// a [cap][H] buffer in expert-sorted order — experts in the listed order, each expert's rows in
// its sorted order. Rows past cap are not moved: the launch then sets ovf[flag] = 1 (and
// ovf[eflag[k]] for an expert whose own count exceeds ecap[k]: its compact output rows
// travel back in an edge of that capacity). No host sync: the counts are the device routing's.
constexpr int kMoePackMaxDest = 8, kMoePackMaxExp = 8;
struct MoePackDest {
  void* buf;                        // [cap][H] compact rows
  int cap, n_exp, flag;
  int experts[kMoePackMaxExp];
  int ecap[kMoePackMaxExp], eflag[kMoePackMaxExp];  // per expert: return-edge capacity / flag (-1: none)
};
struct MoePackArgs {
  MoePackDest d[kMoePackMaxDest];
  int n;
};
// unpack = 0: buf[c] = x[src[j]] (x: token rows); 1: x[j] = buf[c] (x: the expert-sorted rows)
void launch_moe_pack(const void* x, int H, const int32_t* src_rows, const int32_t* offsets, const MoePackArgs& a,
                     int32_t* ovf, int unpack, int max_rows, hipStream_t s);
void launch_moe_combine(const void* expert_out, const int32_t* slot_of, const float* weights, void* y, int M,
                        int topk, int H, const int32_t* range, hipStream_t s);
// X [rows][K] sorted by expert, offsets [E+1], W [E][N][K] -> Y [rows][N]
void launch_grouped_gemm(const void* X, const int32_t* offsets, const void* W, void* Y, int E, int N, int K,
                         int max_rows, int act, hipStream_t s);

// y[m] = r[m] + sum_j w[m,j] * expert_{idx[m,j]}[slot[m,j] - off[idx[m,j]]] over compact per-expert
// outputs whose base addresses are the device array eo_ptrs[E]; topk <= 8
// yn (optional, H <= 8192): also write norm(y) * nw (+ nb) for the next norm (nmode 1 LayerNorm, 2 RMSNorm)
void launch_moe_gather_combine(const unsigned long long* eo_ptrs, const int32_t* idx, const int32_t* slot_of,
                               const int32_t* off, const float* w, const void* r, void* y, int M, int topk, int H,
                               int E, hipStream_t s, void* yn = nullptr, const void* nw = nullptr,
                               const void* nb = nullptr, int nmode = 0, float neps = 1e-5f);

// dst (HBM) <- src (pinned host memory, device-accessible address); bytes % 16 == 0, both
// 16-byte aligned; at most `blocks` workgroups of 256 lanes pull over the host link
void launch_host_pull(const void* src, void* dst, int64_t bytes, int blocks, hipStream_t s);
void launch_delay(double us, hipStream_t s);

// GPT-2 MLP block in one launch (gemm_fused.hip): h = act1(LN(x) W1'^T + b1) (folded norm with
// handed-over row statistics), out = h W2^T + b2 + R (+ row statistics of out into stats_out)
// One-launch pre-norm attention block (attn_block.hip): QKV GEMM with a folded norm, causal
// MHA (head_dim 64), out-proj + bias + residual (+ next-norm row statistics), linked in-launch.
struct AttnBlockArgs {
  const void* x; int ldx;              // block input rows [M][H] (raw: the norm is folded)
  const void* w1; const void* b1;      // derived QKV weight [3H][H], bias' [3H] (or null)
  const float* colsum1;                // colsum(W') [3H]
  const float* ext_stats;              // (sum, sum of squares) of x's rows [M][2], from x's producer
  int ln_mode; float ln_eps;           // 1 LayerNorm, 2 RMSNorm
  void* qkv; int ldqkv;                // workspace [M][3H]
  void* o; int ldo;                    // workspace [M][H]
  const void* wo; const void* bo;      // out-proj [H][H], bias [H] (or null)
  const void* R; int ldr;              // residual [M][H]
  void* out; int ldout;                // block output [M][H]
  float* stats_out;                    // row statistics of out for the next folded norm (or null)
  int M, H, B, S, n_head;
  float scale;
  int* sync;                           // attn_block_sync_ints() ints, zero before the first launch
  int* err;                            // set when a poll exceeds spin_limit
  int spin_limit;
  unsigned long long* stamps = nullptr;  // diagnostic: [grid][4] (item, start, wait done, end) ticks
};
int attn_block_sync_ints(int M, int S, int B, int n_head);
bool attn_block_supported(int M, int H, int B, int S, int n_head, int n_kv_head, int D);
void launch_attn_block(const AttnBlockArgs& p, hipStream_t s);

struct MlpFusedArgs {
  const void* x;
  int ldx;
  const void* w1;
  int ldw1;
  const void* b1;
  const float* colsum1;
  const float* ext_stats;
  int ln_mode;
  float ln_eps;
  int act1;
  void* h;
  int ldh;
  const void* w2;
  int ldw2;
  const void* b2;
  const void* R;
  int ldr;
  void* out;
  int ldo;
  float* stats_out;
  int M, H, F, Hout;
  int* ready;  // [M / 64] arrival counters, zero before the launch (reset by the launch itself)
  int* done;   // [M / 64]
  int* err;    // set if a poll exceeded spin_limit
  int spin_limit;
  // before its poll, each workgroup DMAs its share of its fc2 weight panel (the panel is
  // shared by the XCD's workgroups of that column tile) so phase 2 finds it in the XCD's L2;
  // -1: DLS_MLP_PREFETCH (default on)
  int prefetch_w2 = -1;
};
bool mlp_fused_supported(int M, int H, int F, int Hout, int cus);
void launch_mlp_fused(const MlpFusedArgs& p, hipStream_t s);  // one wave spinning for ``us`` microseconds (loopback.cpp)
