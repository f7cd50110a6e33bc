/* libechohip — C ABI of the MI355X-native Echo-TTS hot path.
 *
 * The reference (sruckh/echo-tts) is pure Python/PyTorch and has no FFI of its own; the boundary it
 * offers is its Python call signatures.  Each entry point below replaces the body of
 * one of those Python functions; the Python host in `echo-tts_amd/` keeps the reference signatures
 * and calls these through ctypes (INTEGRATION.md shows the binding).
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; echo_last_error() gives the text;
 *   - all tensor arguments are raw DEVICE pointers owned by the caller unless a parameter says
 *     "host"; the library never frees caller memory; it owns packed weights, KV caches and
 *     workspaces inside echo_ctx (grown on demand, never inside the sampler's step loop once warm);
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream); all work
 *     is enqueued on it and nothing synchronises unless stated;
 *   - dtype codes: ECHO_F32 = 0, ECHO_BF16 = 1.  "T" below is the context's activation type:
 *     bf16 (production) or f32 (parity mode: fp32 weights, activations and MFMA);
 *   - one echo_ctx per device, not thread-safe (the reference is single-threaded, one job at a time).
 */
#ifndef ECHO_HIP_H
#define ECHO_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define ECHO_F32 0
#define ECHO_BF16 1
#define ECHO_ABI_VERSION 8

typedef struct echo_ctx echo_ctx;

/* Sizes of EchoDiT (reference: inference.py:16-24, model.py:472-559) and of the Fish S1-DAC decode
 * path (autoencoder.py:1144-1192).  head_dim must be 128 for the DiT and its encoders. */
typedef struct {
  int precision;                 /* ECHO_BF16 or ECHO_F32 */
  int latent_size, model_size, num_layers, num_heads, intermediate_size;
  float norm_eps;
  int text_vocab_size, text_model_size, text_num_layers, text_num_heads, text_intermediate_size;
  int speaker_patch_size, speaker_model_size, speaker_num_layers, speaker_num_heads, speaker_intermediate_size;
  int timestep_embed_size, adaln_rank;
  int has_latent_encoder;        /* 0 when the checkpoint was loaded with delete_blockwise_modules (inference.py:28-34) */
  /* DAC decode path.  ABI 8: it runs in the context's `precision` - ECHO_F32: fp32 weights and activations (the path of ABI <= 7, bit for bit);
   * ECHO_BF16: bf16 weights and channels-last bf16 activations on the bf16 MFMA with fp32 accumulation, the reference's own AE dtype
   * (handler.py:345, inference.py:62-66).  The entry points keep their signatures: fp32 latents in, fp32 waveform out. */
  int dac_latent_dim, dac_decoder_dim, dac_n_rates, dac_rates[8];
  int dac_post_layers, dac_post_heads, dac_post_head_dim, dac_post_ffn, dac_post_window;
  int dac_n_up, dac_up_factors[4];
  float dac_norm_eps;
  /* DAC encode path (speaker reference -> latents; autoencoder.py:903-929, 376-464, 117-158): Encoder channel base,
   * strides, transformer layers per block (window dac_enc_window, heads = C / 64, ffn = 3 C), VQ stack sizes.
   * dac_enc_dim == 0: no encode path in this context. */
  int dac_enc_dim, dac_enc_n_rates, dac_enc_rates[8], dac_enc_tlayers[8], dac_enc_window;
  int dac_n_codebooks, dac_codebook_size, dac_codebook_dim, dac_semantic_size;
  /* BASELINE config C5 ("fp8 MFMA weight path for DiT GEMMs"): 1 = the four large linears of every EchoDiT block (QKV+gate,
   * wo, w1|w3, w2) run on OCP e4m3 operands — weights quantised once at echo_finalize_dit with one scale per output row,
   * activations per token row in front of each GEMM — on the block-scaled MFMA at twice the bf16 rate; accumulation, tails,
   * attention, norms and the encoders stay as in the bf16 engine.  precision must be ECHO_BF16. */
  int dit_fp8;
} echo_config;

int echo_abi_version(void);
const char* echo_last_error(echo_ctx* ctx);            /* ctx may be NULL: last error of a failed create */

/* handler.py:323-417 `_load_models` / inference.py:14-47,56-76: context + weights */
int echo_ctx_create(const echo_config* cfg, int device, echo_ctx** out);
void echo_ctx_destroy(echo_ctx* ctx);

/* Register one checkpoint tensor under its reference state-dict name (SURVEY.md §A.5 for EchoDiT;
 * INTEGRATION.md lists the DAC names, which are the reference names with weight-norm folded and the
 * conv kernels reshaped to GEMM form by the Python loader).  `data` may be a host or a device pointer. */
int echo_load_tensor(echo_ctx* ctx, const char* name, const void* data, int dtype, int ndim, const int64_t* shape,
                     int data_on_device);
int echo_finalize_dit(echo_ctx* ctx, void* stream);    /* pack EchoDiT weights for the kernels, drop the raw copies */
/* ABI 8, ECHO_BF16 context: the decode-path tensors are expected as the loader of a bf16 DAC prepares them: every checkpoint tensor
 * rounded to bf16 first, weight-norm folded from the rounded parameters in bf16, conv kernels then reshaped to GEMM form with every decoder channel
 * count zero-padded to a multiple of 64 (the bf16 K step: 96 -> 128), biases and Snake alphas padded with zeros alike.  They are stored as bf16. */
int echo_finalize_dac(echo_ctx* ctx, void* stream);
/* encode-path tensors ("enc.*", prepared by the Python loader: weight-norm folded, conv kernels in GEMM form, codebooks
 * normalised, from_codes operands concatenated; INTEGRATION.md lists them).  Needs echo_finalize_dac first.
 * ABI 8: the encode path keeps fp32 weights and fp32 kernels in an ECHO_BF16 context too (a bf16 VQ argmax flips codes); pass fp32 tensors. */
int echo_finalize_dac_encoder(echo_ctx* ctx, void* stream);

/* Position tables computed by the host with the reference's own expressions (exactness for free):
 * rope: (npos, 64) float2 = (cos, sin) of model.py:9-14 for head_dim 128;
 * ae_rope: (npos, head_dim/2, 2) fp32 copy of the bf16 cache of autoencoder.py:805-813. */
int echo_set_rope_table(echo_ctx* ctx, const void* table_dev, int npos);
int echo_set_ae_rope_table(echo_ctx* ctx, const void* table_dev, int npos);

/* model.py:606-613 EchoDiT.get_kv_cache_text.  ids (B,Tt) int32; key_bias: NULL when every mask is a
 * prefix, else (B,Tt) f32 additive 0/-inf; nkeys_host[b] = 1 + index of the last attended token. */
int echo_encode_text(echo_ctx* ctx, const int32_t* ids, const float* key_bias, const int32_t* nkeys_host, int B, int Tt,
                     void* stream);
/* model.py:615-621 get_kv_cache_speaker.  latent (B,Ts,latent) of T; masks are over the Ts/patch keys. */
int echo_encode_speaker(echo_ctx* ctx, const void* latent, const float* key_bias, const int32_t* nkeys_host, int B, int Ts,
                        void* stream);
/* model.py:623-636 get_kv_cache_latent for the first n_latents (multiple of patch) prefix latents. */
int echo_encode_latent_prefix(echo_ctx* ctx, const void* latent, int B, int n_latents, long row_stride_elems, void* stream);
/* inference.py:408-414 _multiply_kv_cache on the speaker cache (K and V of layers < max_layers) */
int echo_scale_speaker_kv(echo_ctx* ctx, float scale, int max_layers, void* stream);

/* Per-voice cache.  The reference re-encodes the reference voice for every text chunk (handler.py:750-758 ->
 * inference.py:333-340 -> model.py:615-621).  echo_voice_capture copies the context's current speaker cache (K / V / V^T of all
 * layers, key counts, optional key bias) into an object owned by the caller; echo_voice_bind makes it the context's speaker
 * cache again (device copy, bit-identical to a fresh echo_encode_speaker) on any context of the same model, precision and
 * device.  The speaker cache may have batch size 1 while the text cache has B: every row then shares the one voice. */
typedef struct echo_voice echo_voice;
int echo_voice_capture(echo_ctx* ctx, echo_voice** out, void* stream);
int echo_voice_bind(echo_ctx* ctx, const echo_voice* voice, void* stream);
int64_t echo_voice_bytes(const echo_voice* voice);
void echo_voice_destroy(echo_voice* voice);

/* SURVEY.md §8b "echo_workspace_bytes": device bytes of KV caches + workspaces the context currently holds, and a call that
 * grows them for a request geometry up front (B utterances per sampler call, S latents, Tt text tokens, Ts speaker latents,
 * T_dac frames per decode) so that the first request allocates nothing. */
int64_t echo_workspace_bytes(echo_ctx* ctx);
/* fp8 engine (echo_config.dit_fp8, BASELINE config C5): calibration of static activation scales for the two block operands no producer
 * can quantise per row (attention output -> wo, SwiGLU output -> w2); SURVEY.md 8f-4 "fp8 calibration".  echo_fp8_calibrate(ctx, 1)
 * clears the per-block maxima and records, during every forward until echo_fp8_calibrate(ctx, 0), the largest dynamic row scale
 * (amax / 448) each block sees; echo_fp8_calibration copies the 2 * num_layers values out ([2 l] attention output, [2 l + 1] SwiGLU
 * output); echo_fp8_set_static_scales installs 2 * num_layers scales (the caller applies its margin; n = 0: back to dynamic row scales):
 * the attention epilogue and the SwiGLU tail then write the e4m3 operands themselves and both quantisation passes of a block go away.
 * Values beyond 448 * scale saturate.  The reference has no fp8 path: this is this engine's own stated arithmetic (oracle:
 * set_fp8_block_linears(True, act_static=...)). */
int echo_fp8_calibrate(echo_ctx* ctx, int on);
int echo_fp8_calibration(echo_ctx* ctx, float* out, int n);
int echo_fp8_set_static_scales(echo_ctx* ctx, const float* scales, int n);
int echo_reserve_workspace(echo_ctx* ctx, int B, int S, int Tt, int Ts, int T_dac);

/* model.py:563-604 EchoDiT.forward for `rows` = R*B rows that share one timestep.
 * x (rows*S, latent) of T; temb (1, timestep_embed) of T (model.py:27-43 evaluated by the host);
 * row r uses text/speaker KV of batch item r % B; row_text_on/row_spk_on (host, rows) switch the
 * segments per row (the CFG "uncond" rows); v_out (rows*S, latent) fp32. */
int echo_dit_forward(echo_ctx* ctx, const void* x, const void* temb, int rows, int B, int S, int start_pos, int use_latent,
                     const int32_t* row_text_on, const int32_t* row_spk_on, float* v_out, void* stream);

/* ABI 7: the same forward with PER-ROW timesteps (model.py:563-604 takes any t (R,); model.py:27-43): temb (n_t, timestep_embed) of T
 * holds the embeddings of the n_t distinct timesteps, row_t (host, rows) names the one each row uses.  Rows are processed together;
 * only the launches that read the AdaLN modulation run once per run of consecutive rows with equal row_t. */
int echo_dit_forward_t(echo_ctx* ctx, const void* x, const void* temb, int n_t, const int32_t* row_t, int rows, int B, int S, int start_pos,
                       int use_latent, const int32_t* row_text_on, const int32_t* row_spk_on, float* v_out, void* stream);

typedef struct {
  int has_cfg;                   /* inference.py:484 */
  float dt;                      /* fp32 (t_next - t), inference.py:515 */
  int rescale;                   /* inference.py:507-508, coefficients of inference.py:421-423 evaluated by the host */
  float r_inv1mt, r_ratio, r_1mt;
  int kv_unscale_after;          /* inference.py:511-513 */
} echo_step;

typedef struct {
  int B, S, num_steps;
  int start_pos, use_latent;     /* blockwise: inference_blockwise.py:91-94 */
  float cfg_scale_text, cfg_scale_speaker;
  int has_truncation;            /* ABI 7: 0 = truncation_factor is None (init_scale ignored: a zero-initialised struct samples from the
                                  * un-truncated noise); 1 = x_t = x_t * init_scale (inference.py:478-479), a literal 0.0 included */
  float init_scale;              /* truncation_factor; read only when has_truncation != 0 */
  float kv_scale; int kv_max_layers;   /* used by kv_unscale_after steps: multiply by 1/kv_scale */
  const echo_step* steps;        /* host, num_steps entries */
  const void* temb;              /* device, (num_steps, timestep_embed) of T */
} echo_sampler_params;

/* inference.py:427-517 sample_euler_cfg_independent_guidances, from the noise draw on.
 * x_init (B,S,latent) fp32 noise (the host draws it exactly like inference.py:457,477);
 * latent_out (B,S,latent) fp32.  Text/speaker(/latent) KV must have been encoded on this ctx. */
int echo_sample_euler(echo_ctx* ctx, const echo_sampler_params* p, const float* x_init, float* latent_out, void* stream);

/* ---- mixed batches (added under ABI 8; additive: every declaration above keeps its layout and its bits) ----
 * One sampler call whose utterances differ in every reference request parameter (handler.py:426-444, inference.py:428-447) and in
 * their cached voice.  Two parameters stay per call because they set the launch geometry: num_steps and the sequence length S. */
typedef struct {                 /* one utterance of a mixed call; host memory */
  float cfg_scale_text, cfg_scale_speaker;
  int has_truncation; float init_scale;      /* as in echo_sampler_params */
  float kv_scale; int kv_max_layers;         /* used by THIS item's kv_unscale_after step: multiply by 1/kv_scale */
  const echo_step* steps;        /* host, num_steps entries, this item's: has_cfg, dt, rescale coefficients, kv_unscale_after */
} echo_sampler_item;

/* inference.py:427-517 for B utterances with their own parameters: item b of latent_out is what the reference computes for item b
 * with items[b].  `p` supplies B, S, num_steps, start_pos, use_latent and temb (all items share num_steps, hence the t schedule and
 * one modulation table per step); its per-call scalar fields and p->steps are ignored.  The per-item step data goes to the device
 * once, as a num_steps x B table, before the step loop; nothing is allocated or synchronised inside the loop once warm.
 * Row set: a step runs the 3B-row CFG layout when ANY item has CFG at that step (B rows otherwise), which keeps the `row % B` KV
 * addressing.  Cost: an item outside its CFG window still pays for its two un-conditional rows at such a step (they are computed and
 * not used; compacting them away is not done).  An item without CFG at a step takes v_cond unchanged.  An item whose parameters equal
 * those of a uniform echo_sample_euler call gets that call's bits.
 * Fails (non-zero, text from echo_last_error) when B differs from the text cache's batch, 3B > 96 (more than 32 items), items or an
 * item's steps is NULL, any item's steps[i].dt differs from item 0's, or utterances that share a voice slot (speaker cache of batch
 * spkB < B, slot b % spkB) un-scale their speaker KV differently. */
int echo_sample_euler_items(echo_ctx* ctx, const echo_sampler_params* p, const echo_sampler_item* items /* p->B entries */,
                            const float* x_init, float* latent_out, void* stream);
/* inference.py:408-414 per utterance: K, V and transposed V of item b's speaker cache, layers < max_layers_host[b] (-1: all), times
 * scales_host[b], rounded as echo_scale_speaker_kv rounds.  An item with scale 1 keeps its bits untouched.  n is the speaker cache's
 * batch size or a multiple of it; entries that share a voice slot (b % batch) must be equal, anything else fails. */
int echo_scale_speaker_kv_items(echo_ctx* ctx, const float* scales_host, const int32_t* max_layers_host, int n, void* stream);
/* n captured batch-1 voices (host array of n pointers) become this context's speaker cache of batch n: one voice per utterance without
 * running the speaker encoder.  The cache takes the largest key count; item i keeps its own count, and its K / V rows and transposed-V
 * columns beyond it are ZERO-FILLED (a masked key is multiplied by a zero probability; 0 x NaN from an uninitialised tail is not 0).
 * A key bias is carried only if some voice has one; the others get 0 on their keys.  Same checks as echo_voice_bind. */
int echo_voice_bind_items(echo_ctx* ctx, const echo_voice* const* voices, int n, void* stream);

/* ---- per-utterance start positions (additive: every declaration above keeps its layout and its bits; ECHO_ABI_VERSION stays 8) ----
 * Blockwise generation (inference_blockwise.py:59-121) writes block k of an utterance at start_pos = the latents generated so far: the RoPE
 * position of query / self key s is start_pos + s (inference_blockwise.py:91-94 -> model.py:217-232), and the block sees the first
 * ceil(start_pos / patch) keys of the latent-prefix cache (model.py:623-636).  Streams that arrive at different times stand at different
 * blocks; these two calls take ONE START POSITION PER UTTERANCE, so that such streams share a forward and a sampler call.
 *   - item_start_pos: HOST table of B int32; row r of a forward uses item_start_pos[r % B].  It goes to the device once per call.
 *   - latent keys of row r: min(cache length, ceil(item_start_pos[r % B] / patch)).
 *   - echo_encode_latent_prefix is unchanged: encode once up to the LONGEST item's prefix.  The latent encoder is causal, so the keys an item
 *     with a shorter prefix may see are exactly those of its own encode; the rest are masked by count.  The prefix buffer beyond an item's own
 *     prefix must hold finite values (zeros): a masked key is multiplied by a zero probability, and 0 x NaN is not 0.
 *   - an item at position p gets the bits a uniform call with start_pos = p gives it (same B, same caches).
 * Fails (non-zero, echo_last_error; the context stays usable) on a NULL table, a negative position, a position + S past the rope table,
 * 3 B > 96 rows, and on everything the call it extends fails on. */
/* echo_dit_forward_t with a position per KV batch item (model.py:563-604; start_pos of inference_blockwise.py:91-94 per row) */
int echo_dit_forward_pos(echo_ctx* ctx, const void* x, const void* temb, int n_t, const int32_t* row_t, int rows, int B, int S,
                         const int32_t* item_start_pos /* host, B */, int use_latent, const int32_t* row_text_on, const int32_t* row_spk_on,
                         float* v_out, void* stream);
/* echo_sample_euler_items with p->start_pos ignored: item b samples its block at item_start_pos[b] (inference_blockwise.py:59-121, one
 * loop iteration for B streams at once).  The positions' RoPE rows are gathered once, in front of the step loop. */
int echo_sample_euler_items_pos(echo_ctx* ctx, const echo_sampler_params* p, const echo_sampler_item* items /* p->B entries */,
                                const int32_t* item_start_pos /* host, p->B */, const float* x_init, float* latent_out, void* stream);

/* ---- per-utterance lengths (additive: every declaration above keeps its layout and its bits; ECHO_ABI_VERSION stays 8) ----
 * One forward / one sampler call for utterances of DIFFERENT lengths (streams that stand at blocks of different sizes, sentences that
 * need different sequence lengths).  The tensors stay rectangular: (rows or B, S, latent); item b owns the first item_len[b] tokens of
 * its rows, 1 <= item_len[b] <= S, the rest is padding.
 *   - self keys of row r: item_len[r % B].  Position, latent-prefix, text and speaker keys as in the position calls.
 *   - valid output rows of an item depend on nothing at a padding position: not on the caller's x / x_init there (never read; NaN and Inf
 *     included), not on what an earlier call left in the workspace, not on the other items' lengths or contents.
 *   - padding rows of v_out / latent_out are written as zeros; in the sampler x_t stays exactly 0 there through every step.
 *   - all lengths equal to S: the bits of echo_dit_forward_pos / echo_sample_euler_items_pos.
 *   - NOT claimed: that an item of length n inside a longer call has the bits of a uniform call with S = n (other M, other GEMM plans).
 *   - padding is still computed by the GEMMs (cost: S - item_len[b] token rows per item row); the bf16 attention skips blocks of padding queries.
 *   - item_start_pos may be NULL: every item at 0 (forward) / at p->start_pos (sampler).  Both tables go to the device in one copy.
 * Fails (non-zero, echo_last_error; nothing is queued, the context stays usable) on a NULL length table, a length below 1 or above S, a start
 * position plus length past the rope table, 3 B > 96 rows, a context created with dit_fp8 (the e4m3 attention output has no length form),
 * a text or speaker cache built from a key mask that is not a prefix (its per-key bias takes the biased attention kernel, which has no length form),
 * and on everything the position calls fail on. */
int echo_dit_forward_len(echo_ctx* ctx, const void* x, const void* temb, int n_t, const int32_t* row_t, int rows, int B, int S,
                         const int32_t* item_start_pos /* host, B, may be NULL */, const int32_t* item_len /* host, B */, int use_latent,
                         const int32_t* row_text_on, const int32_t* row_spk_on, float* v_out, void* stream);
int echo_sample_euler_items_len(echo_ctx* ctx, const echo_sampler_params* p, const echo_sampler_item* items /* p->B entries */,
                                const int32_t* item_start_pos /* host, p->B, may be NULL */, const int32_t* item_len /* host, p->B */,
                                const float* x_init, float* latent_out, void* stream);

/* ---- per-utterance step counts (additive: every declaration above keeps its layout, its bits and its refusals; ECHO_ABI_VERSION stays 8) ----
 * One sampler call for utterances that run DIFFERENT numbers of Euler steps (a 20-step "fast" request next to a 40-step one).
 *   - item_steps: HOST table of B int32, 1 <= item_steps[b] <= p->num_steps.  p->num_steps = N is the call's maximum: the call runs N iterations.
 *   - items[b].steps has item_steps[b] entries: the item's OWN schedule, what a uniform call of that step count would be given.
 *   - the distinct step counts, in order of first appearance in item_steps, are the call's G groups (G <= 8).  p->temb is a table [N][G] of timestep
 *     embeddings (row i * G + g, timestep_embed wide): entry [i][g] belongs to step i of group g's schedule.  Entries with i >= the group's count are
 *     not used for any result; they must be finite (the host repeats the group's last one).  With G = 1 this is the (num_steps, timestep_embed)
 *     table of the calls above.
 *   - iteration i: item b is ACTIVE while i < item_steps[b] and takes its own step i (CFG window, rescale, dt, speaker-KV un-scaling at its own
 *     step); afterwards it is FINISHED: its x_t is not written again, so latent_out holds the bits it had after its last step.
 *   - the row set of an iteration (3 B rows with CFG, B without) is decided by the ACTIVE items' CFG windows alone.
 *   - the layout stays rectangular: a finished item's rows are still computed (with the modulation of its last step, so every workspace value
 *     stays finite) and nobody reads them - the stated cost, like padding tokens and CFG ride-along rows.  Each group adds one launch of the four
 *     modulation-reading kernels per block and row run: ORDER THE ITEMS SO THAT EQUAL STEP COUNTS ARE ADJACENT (at most 3 G row runs; the host
 *     layer sorts by step count).  Any order is computed correctly.
 *   - item_start_pos / item_len may each be NULL and mean what they mean in echo_sample_euler_items_len; both NULL: every item at p->start_pos with
 *     all S tokens (the layout of echo_sample_euler_items).
 *   - all counts equal to N: the bits of echo_sample_euler_items / _pos / _len for the same tables.
 * Fails (non-zero, echo_last_error; nothing is queued, latent_out is not written, the context stays usable) on a NULL item_steps, a count below 1 or
 * above p->num_steps, two items of one step count whose steps[i].dt differ, more than 8 distinct counts, a context created with dit_fp8, items
 * that share a voice slot (speaker cache of batch spkB < B, slot b % spkB), differ in their step counts and un-scale their speaker KV (their
 * kv_unscale_after steps fall into different iterations; the slot's K / V exist once), and on everything the calls it extends fail on. */
int echo_sample_euler_items_steps(echo_ctx* ctx, const echo_sampler_params* p, const echo_sampler_item* items /* p->B entries */,
                                  const int32_t* item_steps /* host, p->B */, const int32_t* item_start_pos /* host, p->B, may be NULL */,
                                  const int32_t* item_len /* host, p->B, may be NULL */, const float* x_init, float* latent_out, void* stream);

/* ---- compacted row sets: a row-to-item map through the forward (additive: every declaration above keeps its layout, its bits and its refusals;
 * ECHO_ABI_VERSION stays 8) ----
 * The calls above address the text, speaker and latent caches, the positions and the lengths by `row % B`, which forces the rectangular B / 3 B
 * row set on every forward.  These take the rows as a MAP: row r belongs to item row_item[r].
 *   - echo_dit_forward_rows: `rows` is any value in 1..96 and need not be a multiple of B; an item may own zero, one or several rows.  Row r takes the
 *     start position, the length, the latent-prefix count, the text keys and the speaker slot of item row_item[r]; x, row_t, row_text_on,
 *     row_spk_on and v_out stay indexed by the row.  item_start_pos / item_len (B entries, per ITEM) may each be NULL: position 0 / all S tokens.
 *     With the rectangular map (row_item[r] = r % B) the bits of echo_dit_forward_t / _pos / _len.  Two forwards with the same `rows` and the same
 *     runs of row_t agree on any row that has the same item, flags, timestep and x, wherever it stands.
 *   - echo_sample_euler_items_compact: echo_sample_euler_items_steps (same tables, same groups, same temb [N][G], same refusals; item_steps may be
 *     NULL: every item runs p->num_steps) whose iteration i runs ONLY the rows somebody reads: the conditional row of every ACTIVE item, and its
 *     text-uncond and speaker-uncond rows if and only if it has CFG at its own step i.  A finished item contributes nothing.  Row order:
 *     group-major (step-count groups in order of first appearance), inside a group conditional, then text-uncond, then speaker-uncond rows, items
 *     in call order: one launch of the modulation-reading kernels per ACTIVE group.  All distinct row sets of the call are planned on the host
 *     and their tables go to the device in the call's one staged copy, in front of the loop.
 *   - one group and every item in CFG at the same steps: the bits of echo_sample_euler_items_len / _steps.  An item's result does not depend on
 *     the other items' contents while their row sets stay the same.  NOT claimed: that an item has the bits of the rectangular or of a uniform
 *     call (other row counts, other M, other GEMM plans).
 *   - echo_debug_last_row_forwards: the sum of `rows` over the forwards of the last sampler call of ANY sampler entry point (test instrument).
 * Fail (non-zero, echo_last_error; nothing is queued, the context stays usable) on a NULL row_item, an entry outside [0, B), rows outside 1..96,
 * a context created with dit_fp8 (the e4m3 attention output has no row-map form), and on everything the calls they extend fail on. */
int echo_dit_forward_rows(echo_ctx* ctx, const void* x, const void* temb, int n_t, const int32_t* row_t, int rows, int B, int S,
                          const int32_t* row_item /* host, rows; 0 <= row_item[r] < B */, const int32_t* item_start_pos /* host, B, may be NULL */,
                          const int32_t* item_len /* host, B, may be NULL */, int use_latent, const int32_t* row_text_on, const int32_t* row_spk_on,
                          float* v_out, void* stream);
int echo_sample_euler_items_compact(echo_ctx* ctx, const echo_sampler_params* p, const echo_sampler_item* items /* p->B entries */,
                                    const int32_t* item_steps /* host, p->B, may be NULL: all p->num_steps */,
                                    const int32_t* item_start_pos /* host, p->B, may be NULL */, const int32_t* item_len /* host, p->B, may be NULL */,
                                    const float* x_init, float* latent_out, void* stream);
int64_t echo_debug_last_row_forwards(echo_ctx* ctx);

/* inference.py:226-229 ae_decode -> autoencoder.py:1128-1132 DAC.decode_zq, one batch item:
 * latent (T, latent_size) fp32 -> wav (T * hop) fp32.
 * ECHO_BF16 context (ABI 8): the PCA inverse is evaluated in fp32 and rounded to bf16 once (inference.py:227-229), the decoder runs in bf16 and the
 * waveform comes back as fp32 numbers that are bf16-representable (`.float()` of a bf16 result). */
int echo_dac_decode(echo_ctx* ctx, const float* latent, int T, float latent_scale, float* wav_out, void* stream);
/* autoencoder.py:1128-1132 DAC.decode_zq alone: z (T, dac_latent_dim) fp32 CHANNELS-LAST (= z_q[b].T) -> wav (T * hop).
 * ECHO_BF16 context: z is rounded to bf16 first (`z_q.to(fish_ae.dtype)`); output as for echo_dac_decode. */
int echo_dac_decode_zq(echo_ctx* ctx, const float* z, int T, float* wav_out, void* stream);
/* ABI 6: B utterances of T frames each (latent: B x T x latent_size, contiguous) -> wav_out + b * wav_stride (floats).  Same result as B
 * echo_dac_decode calls up to the fp32 summation order of the row-wise GEMMs: the PCA inverse, the post_module transformer and its norm
 * run once on the B * T stacked rows (attention per item and head), the convolution stack per item.  inference.py:226-229 on a batch.
 * ECHO_BF16 context: the same schedule on bf16 rows; items agree with single decodes up to the summation order of the row-wise GEMMs. */
int echo_dac_decode_batch(echo_ctx* ctx, const float* latent, int B, int T, float latent_scale, float* wav_out, int64_t wav_stride, void* stream);
/* Streaming decode (reference: every conv of autoencoder.py:264-331 is causal, gradio_app.py:43 decodes whole
 * utterances): latent (T, latent_size) fp32 are ALL frames generated so far; the window-limited post_module transformer
 * runs over all of them, the convolutional stack only over frames first_frame.. ; wav_out receives (T - first_frame) * 2048
 * samples.  Samples further than the stack's receptive field (< 10 frames) behind first_frame equal the
 * whole-utterance decode; the caller (DACStream in autoencoder.py) discards that context.  ECHO_BF16 context: as echo_dac_decode. */
int echo_dac_decode_tail(echo_ctx* ctx, const float* latent, int T, int first_frame, float latent_scale, float* wav_out, void* stream);
/* The tails of n open streams in one call (additive under ABI 8).  Item i means echo_dac_decode_tail(latent, T, first_frame, ...)
 * followed by dropping the first drop_frames * hop samples (the re-decoded context): the front sees all T frames of that item and no other
 * item's, the convolution stack frames first_frame.. with the single call's left context at every layer, wav_out receives the remaining samples and nothing
 * else is written.  The front runs once on the items' stacked rows, the convolution stack once per layer for a group of items (groups are
 * formed so that the decode buffers stay those of one 640-frame utterance).
 *   - fp32: an item agrees with its single call up to the fp32 summation order of the row-wise GEMMs (other M, other tile plans).
 *   - ECHO_BF16: same schedule; equal bits are NOT claimed for ragged groups (DESIGN.md 3.13 names the kernel), the distance stays inside
 *     half the bf16 decoder's own distance to fp32.
 *   - in front of first_frame every layer sees what echo_dac_decode_tail's taps see there (rows of the item's own front output or zeros,
 *     DESIGN.md 3.13), so the samples right behind a first_frame > 0 equal the single call's as well; DACStream drops them either way.
 *   - an item's samples do not depend on the other items' contents; the caller's memory behind row T of a latent is never read.
 * Fails (non-zero, echo_last_error; nothing is queued, the context stays usable) on n outside 1..32, first_frame outside [0, T),
 * drop_frames outside [0, T - first_frame), T beyond the AE RoPE table, a missing echo_finalize_dac / echo_set_pca. */
typedef struct {
  const float* latent;     /* device, (T, latent_size) fp32: ALL frames of this stream so far */
  int32_t T, first_frame;  /* the convolution stack runs on frames first_frame .. T-1 */
  int32_t drop_frames;     /* leading frames of the tail whose samples are not written (the context) */
  float* wav_out;          /* device, receives (T - first_frame - drop_frames) * hop samples */
} echo_dac_tail_item;
int echo_dac_decode_tail_items(echo_ctx* ctx, const echo_dac_tail_item* items /* host, n */, int n, float latent_scale, void* stream);
/* inference.py:86-99 PCAState: w = pca_components transposed, (dac_latent_dim, latent_size) row-major fp32; mean (dac_latent_dim).
 * The operands stay fp32 in an ECHO_BF16 context as well: the reference computes the PCA inverse in fp32 whatever the AE dtype. */
int echo_set_pca(echo_ctx* ctx, const float* w, const float* mean, int on_device, void* stream);
int echo_dac_hop(echo_ctx* ctx);
/* inference.py:218-224 ae_encode = DAC.encode_zq (autoencoder.py:1080-1126) + PCA projection, one item:
 * audio (n_samples) fp32 device pointer, n_samples a multiple of the frame length (hop * 4 = 2048; the host pads);
 * latent_out (T, latent_size) fp32, T = n_samples / frame; optional codes_out (1 + n_codebooks, T) int32 and
 * zq_out (T, latent_dim) fp32 (channels-last) for parity checks.  PCA operands: echo_set_pca_encode. */
int echo_dac_encode(echo_ctx* ctx, const float* audio, long n_samples, float* latent_out, int32_t* codes_out, float* zq_out,
                    void* stream);
/* w (latent_size, latent_dim) = pca_components, bias (latent_size) = -(pca_mean @ pca_components^T), scale = latent_scale */
int echo_set_pca_encode(echo_ctx* ctx, const float* w, const float* bias, float scale, int on_device, void* stream);

/* ---- single-kernel entry points (unit tests and micro-benchmarks; same kernels the engine launches) ---- */
typedef struct {
  const void* A; const void* W; void* C; void* C2;
  int M, N, K, Npad; int64_t lda, ldw, ldc;
  int taps, tap_base, tap_shift;
  int nbatch, nbi; int64_t a_bo, a_bi, w_bo, w_bi, c_bo, c_bi;
  float acc_scale;
  const void* bias; int64_t bias_bo, bias_bi; int vec_mod;
  float div; int act;
  const void* colscale;
  const void* res; int64_t ldres, res_bo, res_bi;
  const void* snake_alpha;
  int store_main, swiglu;
  int cfg;                       /* plan: 0..4, 6..9 tile configurations (csrc/gemm.hip TileCfg table), 5 = bf16 ping-pong kernel */
  int ksplit; void* ws; int64_t ws_bytes;   /* split-K: fp32 workspace of ksplit * roundup(M,768) * Npad * 4 bytes */
  int split3;                    /* fp32 only: 3 x bf16 MFMA per product (hi/lo operand splitting), ~1e-5 relative error */
  /* ABI 8, dtype ECHO_BF16 with snake_alpha != NULL (the conv forms of the bf16 DAC decoder): acc * acc_scale + bias [+ residual] and the Snake are
   * evaluated in fp32 and each output (C, C2) is rounded to bf16 once, at its store; every other bf16 launch rounds after each step as before */
  int fp8;                       /* dtype ECHO_BF16, cfg 5 only: A and W are e4m3 bytes, y = acc * a_scale[m] * w_scale[n]; K % 128 == 0 */
  const float* a_scale; const float* w_scale;
  /* fused QKV(G) tail (model.py:217-232): the N axis is [q | k | v | gate] x qkv_D; q and k get the per-head RMSNorm (qk_w =
   * [q_norm | k_norm], each qkv_D, eps qk_eps) and interleaved-pair RoPE on heads < rope_heads at position pos0 + (m % qkv_S)
   * (rope: (npos, 64) float2 cos/sin); v is written transposed to vt[(m / qkv_S)][h * 128 + d][m % qkv_S] (pitches vt_ld,
   * vt_row_stride in elements); gate is stored as is.  cfg 0-5 only, qkv_D % 256 == 0. */
  int qkv_mode, qkv_D, qkv_S, rope_heads, pos0; float qk_eps;
  const void* qk_w; const void* rope; void* vt; int64_t vt_ld, vt_row_stride;
  int w_presplit;                /* split3 only: W was reformatted in place by echo_op_presplit_weights (static weights) */
  /* ABI 6, fp8 with a static (calibrated) activation scale: a_scale == NULL -> every A row has the scale a_scale_const (> 0);
   * c8 != NULL (fp8 + swiglu only): the SwiGLU output leaves as e4m3(bf16(out) * c8_inv) bytes at c8 (row pitch c8_ld bytes, % 8 == 0,
   * saturating at +-448) instead of bf16 at C - the A operand of the next fp8 GEMM without a quantisation pass */
  float a_scale_const; void* c8; int64_t c8_ld; float c8_inv;
  int qkv_gate_act;              /* ABI 6, qkv_mode + bf16: the gate section is stored as bf16(sigmoid(bf16(acc))) (v_exp + v_rcp form) - the value the
                                  * attention epilogue derives from a raw gate; pass echo_attn_desc.g_activated = 1 to the attention that reads it */
} echo_gemm_desc;
int echo_op_gemm(int dtype, const echo_gemm_desc* d, void* stream);
/* In-place reformat of an fp32 weight matrix (rows x ld, ld % 32 == 0) for w_presplit: every aligned block of 32 floats becomes
 * 32 bf16 hi = bf16(x) followed by 32 bf16 lo = bf16(x - hi), the values the split3 kernels otherwise compute per fragment.  Results of a
 * split3 GEMM are bit-identical with and without it.  (New in ABI 5; the engine applies it to the Fish S1-DAC decoder's conv weights.) */
int echo_op_presplit_weights(float* w, int64_t rows, int64_t ld, void* stream);
/* bf16 rows -> OCP e4m3 bytes + one fp32 scale per row (amax / 448): the operand format of the fp8 GEMM */
int echo_op_quant_rows_fp8(const void* x, int64_t ldx, void* q, int64_t ldq, float* scale, int rows, int K, void* stream);
/* ABI 7: the fp8 engine's AdaLN-apply (model.py:76-83 on bf16 rows: x_hat * scale1p + shift, rounded to bf16) whose output leaves as
 * e4m3 bytes + one fp32 scale per row (amax / 448) - echo_op_norm(mode 0) followed by echo_op_quant_rows_fp8 in one pass.
 * D % 8 == 0, D <= 4096. */
int echo_op_norm_adaln_fp8(const void* x, int64_t ldx, void* q, int64_t ldq, float* scale, int rows, int D, float eps,
                           const void* scale1p, const void* shift, void* stream);
int echo_op_pack_rows(const void* src, int src_dtype, int64_t src_ld, void* dst, int dst_dtype, int64_t dst_ld, int rows,
                      int cols, int dst_row0, int swiglu_half, void* stream);

typedef struct {
  const void* K; int64_t k_ld, k_row_stride, k_head_stride;
  const void* Vt; int64_t vt_ld, vt_row_stride, vt_head_stride;
  const int32_t* nkeys; const float* bias; int64_t bias_row_stride; int kv_mod;
} echo_attn_seg;
typedef struct {
  const void* Q; int64_t q_ld, q_row_stride;
  void* O; int64_t o_ld, o_row_stride;
  const void* G; int64_t g_ld, g_row_stride;
  int S, H, rows, nseg; echo_attn_seg seg[4]; int causal; float scale;
  void* prof;                    /* diagnostic build only: (workgroups*4, 4) uint64 cycle sums; NULL normally */
  void* redo;                    /* optional device scratch of rows * H * ceil(S / 256) int32 for the fast kernel's range report (DESIGN.md
                                    3.2); NULL: the library uses a buffer of its own per host thread and device */
  /* ABI 6: O8 != NULL -> the (gated) output is written as e4m3(bf16(out) * o8_inv) bytes to O8 (same indexing as O, pitches in bytes,
   * o8_ld % 4 == 0, saturating) INSTEAD of bf16 to O: wo's fp8 operand under a static activation scale (echo_fp8_set_static_scales) */
  void* O8; int64_t o8_ld, o8_row_stride; float o8_inv;
  int g_activated;               /* ABI 6: G already holds bf16(sigmoid(gate)) (echo_gemm_desc.qkv_gate_act): the epilogue only multiplies */
} echo_attn_desc;
int echo_op_attention_bf16(const echo_attn_desc* d, void* stream);
/* The same launch under a per-row length table (additive under ABI 8): qlen_dev[r] (device, d->rows entries) is the number of
 * leading queries of row r that anybody reads.  A query block that starts at or beyond it is not computed: its O block comes back as zeros.
 * The self segment's key counts are the caller's (the engine passes nkeys = qlen); K / Vt at padding positions must be finite.  A NULL
 * table, causal, O8, prof or a per-key bias together with a table fail with a status and a message (echo_last_error(NULL)). */
int echo_op_attention_bf16_len(const echo_attn_desc* d, const int32_t* qlen_dev, void* stream);
/* The same launch under a row map (additive under ABI 8): row_item_dev[r] (device, d->rows entries) is the batch item whose shared
 * KV row r reads: in every segment with kv_mod > 0 the KV row - and the row of the per-key bias - is row_item_dev[r] % kv_mod.  The self segment
 * (kv_mod 0), nkeys, qlen_dev, Q, O and G stay indexed by r.  Row r has the bits of the launch above run on KV physically gathered for row r.
 * qlen_dev may be NULL.  A NULL map, causal, O8 or prof fail with a status and a message (echo_last_error(NULL)). */
int echo_op_attention_bf16_rows(const echo_attn_desc* d, const int32_t* row_item_dev, const int32_t* qlen_dev /* may be NULL */, void* stream);

int echo_op_norm(int dtype, int mode, const void* x, int64_t ldx, void* y, int64_t ldy, int rows, int D, float eps,
                 const void* w0, const void* w1, void* stream);
int echo_op_headnorm_rope(int dtype, void* x, int64_t ldx, int64_t t_stride, int nt, int rows, int S, int H, const void* w,
                          int64_t w_stride, float eps, int do_norm, int rope_heads, const void* rope, int pos0, int pos_mul,
                          void* stream);
int echo_op_transpose_heads(int dtype, const void* v, int64_t ldv, void* vt, int64_t vt_ld, int64_t vt_b_stride, int B, int S,
                            int H, int HD, void* stream);

/* -- the Fish S1-DAC's small kernels and the two softmaxes, one launch each (additive: ECHO_ABI_VERSION stays 8; tests/test_gpu_dac_kernels.py).
 * Every wrapper refuses NULL operands, a dtype other than ECHO_F32 / ECHO_BF16 and the shapes named below with a non-zero status and launches
 * nothing.  Pitches (ld*) are in elements.  "rows of S" = the causal padding restarts every S rows (one batch item).
 *
 * ConvNeXtBlock front half (autoencoder.py:362-364): y[t][c] = LayerNorm_C(b[c] + sum_k w[c][k] * x[t - 6 + k][c]) over the taps inside t's own
 * item, T rows of S.  x, y, w (C, 7), b, lnw, lnb have `dtype`; bf16 rounds the conv output to bf16 before the LayerNorm and the result once.
 * T >= 1, S >= 1, C % 4 == 0, 4 <= C <= 1024, ldx, ldy >= C and % 4 == 0.  Rows of an earlier item that the padding hides are not read. */
int echo_op_dac_dwconv_ln(int dtype, const void* x, int64_t ldx, void* y, int64_t ldy, int T, int S, int C, const void* w, const void* b,
                          const void* lnw, const void* lnb, float eps, void* stream);
/* Decoder tail (autoencoder.py:994): y_f32[t] = tanh(bias + sum_kk w[kk] . x[t - (k - 1) + kk]) over the taps inside t's own item, T rows of S.
 * x, w (k, C) have `dtype`, y is fp32 in both (bf16: the pre-activation and the result are rounded to bf16).
 * T >= 1, S >= 1, C % 4 == 0, 4 <= C <= 128, 1 <= k <= 8, ldx >= C and % 4 == 0. */
int echo_op_dac_conv_out_tanh(int dtype, const void* x, int64_t ldx, float* y_f32, int64_t T, int S, int C, int k, const void* w, float bias,
                              void* stream);
/* Snake (autoencoder.py:96-102), fp32: y[r][c] = x + sin(alpha[c] * x)^2 / (alpha[c] + 1e-9).  rows, C >= 1, ldx, ldy >= C. */
int echo_op_dac_snake(const float* x, int64_t ldx, float* y, int64_t ldy, int64_t rows, int C, const float* alpha, void* stream);
/* Interleaved-pair RoPE of the window transformers (autoencoder.py:815-826), in place on columns [0, H * HD) of x: row r has position r % S in
 * cache (positions, HD / 2, 2) fp32 cos | sin.  The four products and the two sums are rounded separately (no FMA), bf16 once at the store.
 * rows, S, H >= 1, HD >= 2 and even, ldx >= H * HD; the cache has at least min(rows, S) positions. */
int echo_op_dac_rope(int dtype, void* x, int64_t ldx, int rows, int S, int H, int HD, const float* cache, void* stream);
/* Encoder head (autoencoder.py:917), fp32: y[t][c] = b[c] + sum_kk w[c][kk] * x[t - (k - 1) + kk] (x = 0 before the first sample, which is
 * not read), s[t][c] = Snake(y[t][c], alpha[c]); y and s share the pitch ld.  T, k >= 1, C % 4 == 0, C >= 4, ld >= C and % 4 == 0. */
int echo_op_dac_conv_in_snake(const float* x, int64_t T, int C, int k, const float* w, const float* b, const float* alpha, float* y, float* s,
                              int64_t ld, void* stream);
/* VectorQuantize.decode_latents (autoencoder.py:145-158), codebook_dim 8, fp32: idx[t] = the first argmax over the codes of
 * -|e^ - c^|^2 (e^ = e[t] / max(|e[t]|, 1e-12), c^ = cbn, the L2-normalised codebook), zst[t][0..7] = e + (cb[idx] - e), gath[t][0..7] = cb[idx].
 * T, size >= 1, lde, ld_zst, ld_g >= 8; cbn 16-byte aligned. */
int echo_op_dac_vq_argmax(const float* e, int64_t lde, int T, const float* cbn, const float* cb, int size, int32_t* idx, float* zst,
                          int64_t ld_zst, float* gath, int64_t ld_g, void* stream);
/* Row softmax in place on scores s (total_rows, ld); row r is query r % rows_per_batch of batch r / rows_per_batch.  Columns ncols..ncols_pad-1
 * come back as zeros, columns beyond ncols_pad stay.  causal: keys > query are masked; window > 0 also masks keys < query - window + 1.
 * ECHO_F32 (softmax_f32_kernel): bias (may be NULL) adds bias[(batch / heads_per_bias_row) * bias_batch_stride + c] first (-inf masks a key).
 * ECHO_BF16 (softmax_window_bf16_kernel): bias == NULL and causal == 1 are required; only the window's columns are read.
 * rows_per_batch >= 1, total_rows a positive multiple of it, 1 <= ncols <= ncols_pad <= ld, heads_per_bias_row >= 1. */
int echo_op_softmax(int dtype, void* s, int64_t ld, int rows_per_batch, int64_t total_rows, int ncols, int ncols_pad, const float* bias,
                    int64_t bias_batch_stride, int heads_per_bias_row, int causal, int window, void* stream);

/* ---- on-device post-processing; `*_host` arguments are host arrays of n <= 64 entries ----
 * inference.py:288-296 find_flattening_point for B latents (T, W) fp32 (item_stride floats apart): out_dev[b] = first frame whose
 * zero-extended `window` frames have unbiased std < std_threshold and |mean - target| < 0.1, T if none. */
int echo_op_find_flattening_point(const float* latent, int64_t item_stride, int B, int T, int W, int window, float target,
                                  float std_threshold, int32_t* out_dev, void* stream);
/* handler.py:199-211: out_dev[c] = number of trailing samples below `threshold` among the last min(len, max_window) of chunk c */
int echo_op_trailing_quiet(const float* const* chunks_host, const int64_t* lens_host, int n, int max_window, float threshold,
                           int32_t* out_dev, void* stream);
/* handler.py:126-170 crossfade_chunks over chunks already trimmed / zero-extended by handler.py:213-232: chunk i supplies
 * len[i] samples from output position start[i] (the first valid[i] from src[i], zeros after), overlapping chunk i + 1 by
 * overlap[i] samples mixed as result * linspace(1,0,n) + next * linspace(0,1,n). */
int echo_op_assemble_chunks(const float* const* src_host, const int64_t* start_host, const int64_t* len_host, const int64_t* valid_host,
                            const int32_t* overlap_host, int n, float* out_dev, int64_t total, void* stream);

/* ABI 7, SURVEY.md 8f-4 `load_audio` (inference.py:104-113: torchaudio.functional.resample to 44.1 kHz): polyphase FIR resampling of one mono
 * signal on the device.  bank (up, taps) fp32 = the windowed-sinc filters of the `up` output phases (built by the host:
 * echo_tts_amd.inference.sinc_resample_bank restates torchaudio's published sinc_interp_hann kernel); out[f * up + p] =
 * sum_k bank[p][k] * x[f * down + k - width], x = 0 outside [0, n).  The caller crops to ceil(up * n / down) samples. */
int echo_op_resample(const float* x_dev, int64_t n, const float* bank_dev, int taps, int up, int down, int width, float* out_dev, int64_t n_out,
                     void* stream);

/* test hook: copy one DiT layer's cached K and V (which: 0 text, 1 speaker, 2 latent) as fp32 (B, T, model_size);
 * K is post-k_norm(/RoPE), V as projected.  Synchronous.  *B_out / *T_out receive the cache geometry. */
int echo_debug_get_kv(echo_ctx* ctx, int which, int layer, float* k_out, float* v_out, int* B_out, int* T_out);

/* ABI 7, test instrument ("does the parity test have teeth?"): the nth plain-store GEMM launch with M >= 512 and N >= 512 from now on
 * (in an EchoDiT forward: in_proj, then wo and w2 of every block, whatever tile kernel runs them) has its output tile (rows 256..511,
 * columns 256..511) negated right after the launch - what one wrong entry in a kernel's tile walk would produce.  nth = 0 disarms.
 * tests/test_gpu_engine.py shows that its full-depth checks reject such a forward. */
int echo_debug_corrupt_tile(echo_ctx* ctx, int nth);
/* test instrument of the same kind for echo_sample_euler_items_steps, ONE-SHOT like the countdown above: on != 0 -> the NEXT accepted call builds
 * its (step, item) table WITHOUT the `done` flag, so a finished item is updated again with its last step's entry - what an update kernel that
 * ignored the flag would do - and disarms the instrument; every later call is a normal one.  0 disarms at once.
 * tests/test_gpu_item_steps.py shows that its frozen-item check rejects such a call. */
int echo_debug_item_steps_ignore_done(echo_ctx* ctx, int on);

/* timing of the engine's phases, filled by the last echo_sample_euler / echo_dac_decode when
 * echo_set_profiling(ctx, 1) was called (HIP events on the caller's stream; adds synchronisation) */
typedef struct {
  float ms_mod, ms_steps, ms_total;
  float ms_gemm_sum; int n_gemm;   /* sum / count of gemm_nt launch durations of the last profiled run */
  /* the dominant kernel alone: gemm_pp_kernel launches (plan cfg 5) of that run, their HIP-event time on the launch
     stream and their algorithmic FLOPs 2 * M * N * K * taps (bench.py "roofline") */
  float ms_pp_sum; int n_pp;
  double flops_pp;
  float ms_attn_sum; int n_attn;   /* attn_kernel launches of that run (HIP events on the launch stream) */
} echo_profile;
int echo_set_profiling(echo_ctx* ctx, int on);
int echo_get_profile(echo_ctx* ctx, echo_profile* out);

#ifdef __cplusplus
}
#endif
#endif
