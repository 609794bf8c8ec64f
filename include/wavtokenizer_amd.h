/*
 * wavtokenizer_amd.h — C-ABI of libwavtok_hip.so (MI355X / gfx950).
 *
 * The reference (Rita-zi/WavTokenizer) is 100 % Python; it has no FFI boundary of its own.
 * The drop-in boundary is the Python class decoder/pretrained.py:32 `WavTokenizer`; this
 * library is what our same-named class binds (ctypes) underneath.  Each entry point cites the
 * reference function whose work it performs.  Conventions:
 *
 *   - plain C: raw device pointers, explicit sizes, `void* stream` = hipStream_t
 *     (NULL = the null stream).  No torch types.
 *   - every function returns 0 on success, a negative wt_status otherwise; nothing throws
 *     across the ABI; wt_last_error() gives a thread-local message.
 *   - the caller owns every buffer, including the workspace (size from
 *     wt_plan_workspace_bytes).  Kernels are enqueued on `stream`; nothing synchronises,
 *     allocates or frees inside wt_encode / wt_decode / wt_codes_to_features.
 *   - the workspace of a plan may hold anything when a call starts (another call's activations, NaNs, another tenant's
 *     bytes): every word that can reach a result has been written by an earlier step of the SAME call, so a call's
 *     outputs are a function of its inputs alone.  Its address must be a multiple of 256 bytes: stage buffers sit at multiples of 256
 *     bytes from its start, and the kernels rely on that for their 16-byte fills, vector loads and buffer loads, the
 *     128-byte split-f16 groups and 256-byte rows.  Every run entry point of a plan (wt_encode, wt_encode_mixed, wt_decode,
 *     wt_decode_mixed, wt_decode_codes, wt_decode_codes_mixed, wt_head, wt_seanet_decode, wt_unit_run) returns
 *     WT_ERR_INVALID for any other address, before it launches anything.  The library never writes outside
 *     [workspace, workspace + wt_plan_workspace_bytes).
 *   - a wt_model is immutable after creation (folded + packed weights in HBM) and may be shared
 *     by host threads.  A wt_plan may be shared too: host calls on one plan are serialised by a
 *     per-plan lock (they only enqueue), and calls that may be in flight on the GPU at the same
 *     time (two streams) need a plan and a workspace each (stage buffers and the call's status
 *     word live in the workspace).  Calls that launch the persistent LSTM kernel are chained per
 *     device by the library: one made on another stream than the previous one first waits on the
 *     GPU for that previous call (two such launches must never share the CUs).
 *   - a call that fails ON THE DEVICE (wt_status_bits) never hands out plausible data: the guard
 *     step that ends every plan overwrites its outputs (codes = -1, floats = NaN), and the next
 *     host call on ANY plan of the same model returns the matching error once, without running
 *     (wt_plan_status, wt_model_status): a caller that makes a new plan per input length still meets it.
 *   - activations inside the library are time-major [clip][frame][channel] fp32; the API
 *     tensors keep the reference's layouts (wav (B,T); features (B,512,L); codes (K,B,L) int64).
 *   - a decoder that holds codes calls wt_decode_codes / wt_decode_codes_mixed: the codebook rows are gathered straight into
 *     the plan's first operand, and no (B,512,L) feature tensor exists (wt_codes_to_features + wt_decode computes the same bits).
 */
#ifndef WAVTOKENIZER_AMD_H
#define WAVTOKENIZER_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    WT_OK = 0,
    WT_ERR_INVALID = -1,      /* bad argument / unsupported configuration */
    WT_ERR_MISSING_TENSOR = -2,
    WT_ERR_SHAPE = -3,
    WT_ERR_HIP = -4,          /* a HIP runtime call failed */
    WT_ERR_NOT_INITED = -5,   /* codebook buffer `inited` != 1 (core_vq.py:140-151 would run k-means) */
    WT_ERR_RANGE = -6,        /* an EARLIER call on this model met a value outside the f16 range of the split-f16 form; its
                                 outputs were poisoned; re-plan with WT_PLAN_FLAG_FP32_GEMM and repeat both calls */
    WT_ERR_LSTM_SYNC = -7,    /* an EARLIER call's persistent LSTM lost co-residency (a step barrier timed out); its outputs
                                 were poisoned; every plan of the model now runs the LSTM one launch per step: repeat both calls */
    WT_ERR_INDEX = -8         /* a code outside [0, bins) (F.embedding raises IndexError: decoder/pretrained.py:236) */
} wt_status;

/* Device-side failure bits of a call (wt_plan_status). */
enum wt_status_bits {
    WT_STATUS_BIT_LSTM = 1,   /* persistent LSTM: a step barrier timed out */
    WT_STATUS_BIT_RANGE = 2,  /* an S32 (split-f16) producer met |v| >= 65504 */
    WT_STATUS_BIT_LENGTH = 4  /* wt_decode_mixed: a clip length outside [1, Lpad] (the next call returns WT_ERR_INVALID once) */
};

/* Architecture: the YAML keys decoder/pretrained.py:81-92 (from_hparams0802) reads. */
typedef struct {
    int32_t n_ratios;
    int32_t ratios[8];               /* `dowmsamples`, decoder order as written in the YAML */
    int32_t vq_bins;                 /* 4096 */
    int32_t num_quantizers;          /* 1 */
    int32_t input_channels;          /* 512 */
    int32_t dim;                     /* 768 */
    int32_t intermediate_dim;        /* 2304 */
    int32_t num_layers;              /* 12 */
    int32_t adanorm_num_embeddings;  /* 4 */
    int32_t n_fft;                   /* 2400 / 1280 */
    int32_t hop_length;              /* 600 / 320 */
    int32_t padding_same;            /* ISTFT padding (spectral_ops.py:33-47): 1 = "same" (every YAML; audio = L * hop samples), 0 = "center"
                                        (torch.istft(center=True): (L - 1) * hop samples per clip, L >= 2) */
} wt_arch;

/* One named fp32 host array of a checkpoint `state_dict` (keys: SURVEY.md Appendix A). */
typedef struct {
    const char*  name;
    const float* data;    /* host pointer, fp32, contiguous */
    int64_t      numel;
} wt_tensor;

typedef struct wt_model wt_model;
typedef struct wt_plan  wt_plan;

typedef enum {
    WT_PLAN_ENCODE = 0,          /* audio (B,T)       -> features (B,512,L) + codes (1,B,L)  */
    WT_PLAN_DECODE = 1,          /* features (B,512,L) -> audio (B, L*hop)                     */
    WT_PLAN_SEANET_DECODER = 2,  /* features (B,512,L) -> audio (B,1,L*hop): encodec.decoder   */
    WT_PLAN_HEAD = 3,            /* backbone output (B,L,dim) -> audio (B, L*hop): model.head   */
    WT_PLAN_UNIT_LSTM = 4,       /* unit tests: x [B][L][512] -> SLSTM(x) [B][L][512], time-major (wt_unit_run) */
    WT_PLAN_DECODE_MIXED = 5,    /* features (B,512,Lpad) + lengths (B) -> audio (B, wave_len(Lpad)): wt_decode_mixed; `len` = Lpad */
    WT_PLAN_DECODE_CODES = 6,    /* codes (K,B,L) -> audio (B, L*hop): wt_decode_codes; WT_PLAN_DECODE with its first step (the transpose
                                    of the features) replaced by the gather of the codebook rows; `len` = L */
    WT_PLAN_DECODE_CODES_MIXED = 7,  /* codes (K,B,Lpad) + lengths (B) -> audio (B, wave_len(Lpad)): wt_decode_codes_mixed; `len` = Lpad */
    WT_PLAN_QUANTIZE = 8         /* features (B,512,L) -> codes (n_q,B,L): greedy residual VQ with the call's n_q codebooks
                                    (wt_quantize); `len` = L.  Takes FP32_GEMM, GRAPH, KEEP_STAGES and RANGE_REPORT */
} wt_plan_kind;

enum {
    WT_PLAN_FLAG_KEEP_STAGES = 1,  /* never alias stage buffers and snapshot the in-place residual stream (debug taps; bigger
                                      workspace).  The kernels are the ones the default plan launches: taps of the shipped path;
                                      a tap may therefore hold S32-encoded and / or ELU-applied data (wt_plan_buffer_info) */
    WT_PLAN_FLAG_UNFUSED = 16,     /* debug twin: unfused stages, raw fp32 tensors between them (first conv, three-GEMM
                                      resblocks, consumer-side ELU); with FP32_GEMM it is the plain fp32 restatement */
    WT_PLAN_FLAG_STEP_LSTM = 4,    /* LSTM as one launch per time step instead of the persistent per-XCD kernel */
    WT_PLAN_FLAG_GRAPH = 8,        /* small batches: the second call in a row with the same buffers records the plan's
                                      launches as a hipGraph, later calls with those buffers replay it (one
                                      hipGraphLaunch on the caller's stream); any other call launches directly.  Such a
                                      plan must not be run from two host threads at once */
    WT_PLAN_FLAG_FP32_GEMM = 2,    /* every dense layer on the fp32 MFMA chain; default: the fp32-equivalent
                                      split-f16 kernel (3 f16 MFMAs per product, fp32 accumulate) where covered */
    WT_PLAN_FLAG_RANGE_REPORT = 32,/* diagnostic: behind every step, the largest magnitude held by each S32 (split-f16) buffer the
                                      step touches is measured (wt_plan_range_report): the head-room of every dense layer's
                                      operands below the f16 limit 65504.  Costs a pass per buffer; never graph-replayed */
    WT_PLAN_FLAG_MIXED_LENGTH = 64,/* WT_PLAN_ENCODE: clips of different lengths in one call (wt_encode_mixed); `len` is the padded
                                      length.  Only the shipped route takes it: refused together with UNFUSED, FP32_GEMM,
                                      KEEP_STAGES or RANGE_REPORT, with the encoder site on fp32, for weights without S32 copies,
                                      or for a model whose first encoder ratio (the last of `ratios`) is neither 2 nor 4: the
                                      stage-1 kernel that holds the down conv is the one that takes per-clip lengths */
    WT_PLAN_FLAG_F16_GEMM = 128,   /* the decode kinds (WT_PLAN_DECODE, _MIXED, _CODES, _CODES_MIXED): half-precision inference mode for
                                      callers that hold codes and want audio.  Every dense layer that runs on split-f16 operands
                                      multiplies their f16 hi halves alone: one f16 MFMA per product instead of three, fp32
                                      accumulate, operands rounded to f16 (waveform error near 1e-3 relative instead of 1e-5).
                                      Buffers, producers and weights are those of the default plan; a range site on fp32 stays
                                      on the fp32 chain.  Combines with KEEP_STAGES, RANGE_REPORT and GRAPH; refused (WT_ERR_INVALID)
                                      for every other plan kind and together with FP32_GEMM or UNFUSED */
    WT_PLAN_FLAG_RVQ = 256         /* WT_PLAN_ENCODE: the plan's VQ tail is greedy residual VQ over up to num_quantizers codebooks
                                      (wt_encode_rvq, wt_encode_rvq_mixed): codes (n_q,B,L) alone, n_q an argument of the call.
                                      The encoder in front of it is the plan's own; combines with every flag an encode plan takes,
                                      WT_PLAN_FLAG_MIXED_LENGTH included.  The first creation on a model builds the S32 copies and
                                      |e|^2 tables of codebooks 1 .. num_quantizers - 1 (wt_model_codebook_tables) */
};

/* Range sites: the units in which a plan can leave the split-f16 form on its own (wt_plan_create_ex, wt_plan_range_sites).
 * Every S32 tensor is produced and consumed inside one site.  Bit i of a site mask = site i. */
enum wt_range_site {
    WT_SITE_ENCODER = 0,       /* the whole encode plan: SEANetEncoder + VQ (encoder/modules/seanet.py:66-144) */
    WT_SITE_BB_EMBED = 1,      /* backbone.embed (decoder/models.py:177) */
    WT_SITE_RES0 = 2, WT_SITE_RES1 = 3,   /* pos_net ResnetBlocks (decoder/models.py:19-78) */
    WT_SITE_ATTN = 4,          /* AttnBlock (decoder/models.py:80-127) */
    WT_SITE_RES2 = 5, WT_SITE_RES3 = 6,
    WT_SITE_CNX0 = 7,          /* ConvNeXtBlock i = WT_SITE_CNX0 + i (decoder/modules.py:8-60), i < 32 */
    WT_SITE_HEAD = 40,         /* final_layer_norm output + ISTFTHead (decoder/heads.py:24-67) */
    WT_SITE_SEANET_DECODER = 41
};

const char* wt_last_error(void);
const char* wt_version(void);

/* Replaces: WavTokenizer.from_pretrained0802's load_state_dict (decoder/pretrained.py:95-114)
 * plus the weight_norm pre-forward hook of every SConv1d (encoder/modules/conv.py:25-34), done
 * once here: w = g * v / ||v||.  Copies, folds and packs the weights into HBM on `device`.
 * Architectures taken: four ratios of 1 .. 16 each (a down conv has 2 * ratio taps, the GEMM kernels gather 32); num_quantizers 1 .. 32; input_channels 512; dim 256, 512, 768 or 1024;
 * intermediate_dim a multiple of 32; num_layers 1 .. 32; adanorm_num_embeddings >= 1; vq_bins a multiple of 4; n_fft % 4 == 0,
 * a multiple of hop_length with n_fft - hop_length even.  Anything else is refused here (and by wt_model_create_packed and
 * wt_packed_info) with WT_ERR_INVALID and a message that names the field, before any HIP call: an architecture that loads has
 * kernels for every step of every plan. */
int  wt_model_create(const wt_arch* arch, const wt_tensor* tensors, int32_t n_tensors, int32_t device,
                     wt_model** out);
void wt_model_destroy(wt_model* m);

/* Packed weight image ("a packed on-disk weight format, folded, pre-tiled, for fast start"): everything
 * wt_model_create computes and leaves in HBM — weight-norm folded conv weights in [Cout][tap][Cin], LSTM gate-row
 * packings, the packed ISTFT head and inverse-DFT basis, the S32 split copies with their per-tensor scales —
 * behind a header (magic, layout version, the wt_arch, a hash of both, a hash of everything behind the header).
 * wt_model_create_packed allocates, uploads and fixes up pointers: nothing is folded, packed or split again (replaces
 * the load_state_dict + per-forward weight_norm of decoder/pretrained.py:95-114 a second time over).  The file is not
 * trusted: sizes are checked without wrap-around, element counts are bounded, every pointer offset must lie inside
 * its allocation, and the content hash must match before anything is uploaded.  wt_packed_info validates a header
 * and wt_packed_verify the whole image (bounds + content hash) without a GPU. */
size_t wt_model_export_bytes(const wt_model* m);
int  wt_model_export(const wt_model* m, void* buf, size_t n);
int  wt_packed_info(const void* buf, size_t n, wt_arch* arch, int32_t* version, uint64_t* arch_hash);
int  wt_packed_verify(const void* buf, size_t n);
/* exact length of the image that starts at buf (wt_model_export_bytes is an upper bound); 0 when the header is not valid */
size_t wt_packed_bytes(const void* buf, size_t n);
int  wt_model_create_packed(const void* buf, size_t n, int32_t device, wt_model** out);
int  wt_model_hop(const wt_model* m);                 /* prod(ratios) */
/* 1 while the model's plans may launch the persistent LSTM kernel (a 256-CU device and no lost-co-residency report so far) */
int  wt_model_persistent_lstm(const wt_model* m);
/* What the library sees of a device: compute units, whether it is gfx950 (wt_model_create refuses anything else), whether
 * the persistent LSTM can run there (256 CUs = 8 XCDs x 32; a compute partition runs the launch-per-step kernel and sizes
 * every persistent launch by its own CU count). */
int  wt_device_info(int32_t device, int32_t* compute_units, int32_t* is_gfx950, int32_t* persistent_lstm);
int64_t wt_model_weight_bytes(const wt_model* m);     /* packed fp32 bytes resident in HBM */

/* A plan fixes (kind, B, T or L): kernel launch list + workspace layout.
 * `len` = T (samples) for WT_PLAN_ENCODE, L (frames) for every other kind. */
int    wt_plan_create(const wt_model* m, int32_t kind, int32_t B, int64_t len, int32_t flags, wt_plan** out);
/* ... with a mask of range sites (wt_range_site) that keep fp32 operands and run their GEMMs on the fp32 MFMA chain while
 * every other site stays on the split-f16 kernel: the answer to WT_ERR_RANGE that costs one block, not the model. */
int    wt_plan_create_ex(const wt_model* m, int32_t kind, int32_t B, int64_t len, int32_t flags, uint64_t fp32_sites,
                         wt_plan** out);
void   wt_plan_destroy(wt_plan* p);
size_t wt_plan_workspace_bytes(const wt_plan* p);
int64_t wt_plan_frames(const wt_plan* p);             /* L = ceil(T / hop) (conv.py:54-61) */
int    wt_plan_num_launches(const wt_plan* p);
/* calls of this plan that were served by a graph replay (WT_PLAN_FLAG_GRAPH); 0 for a plan without the flag */
int64_t wt_plan_graph_replays(const wt_plan* p);
/* Debug taps: byte offset / element count of a named stage buffer inside the workspace. */
int    wt_plan_find_buffer(const wt_plan* p, const char* name, size_t* offset, size_t* numel);
/* ... and what it holds: format bit 0: the S32 split-f16 encoding (every 32 values of a row = 128 bytes
 * [32 x f16 hi | 32 x f16 lo], value = hi + lo * 2^-11) instead of fp32; bit 1: elu() of the reference's tensor. */
int    wt_plan_buffer_info(const wt_plan* p, const char* name, size_t* offset, size_t* numel, int32_t* format);
/* Device-side failure bits (wt_status_bits) that calls on this plan have reported since the last clear.  The bits of
 * a call are visible once its stream work has completed: synchronise first to learn about the call just made.
 * clear != 0 consumes them together with the model's word (and switches the model to the launch-per-step LSTM after
 * WT_STATUS_BIT_LSTM); bits left unconsumed make the next wt_encode / wt_decode / ... return WT_ERR_LSTM_SYNC /
 * WT_ERR_RANGE once. */
int    wt_plan_status(const wt_plan* p, int32_t* bits, int32_t clear);
/* Which range sites of this plan reported WT_STATUS_BIT_RANGE since the last clear (a site downstream of the first one
 * that overflowed usually reports too: infinities propagate; put the LOWEST set site on fp32 and run again). */
int    wt_plan_range_sites(const wt_plan* p, uint64_t* sites, int32_t clear);
/* WT_PLAN_FLAG_RANGE_REPORT plans, after a call: entry `index` of the report = (step name, S32 buffer name, largest
 * magnitude found in that buffer right behind that step; +inf if a value left the f16 range).  Synchronises the device on the
 * first query after a call.  Returns WT_ERR_INVALID past the last entry. */
int    wt_plan_range_report(const wt_plan* p, int32_t index, const char** step, const char** buffer, float* amax);
/* The same bits collected over ALL plans of the model (each plan's guard step reports into this word too, and it
 * outlives plans that were destroyed): what the next call on any plan of the model will consume. */
int    wt_model_status(const wt_model* m, int32_t* bits, int32_t clear);
/* 1 when every GEMM weight fits the split-f16 form; 0: all plans of this model run the fp32 MFMA chain. */
int    wt_model_split_ok(const wt_model* m);
int    wt_plan_buffer_name(const wt_plan* p, int32_t index, const char** name);

/* Measurement hook (bench.py's roofline leg; no counterpart in the reference): HIP events are
 * recorded on the call's stream around every step whose name contains `name_substr` ("" / NULL
 * turns it off).  A leading '@' ("@cnx.pwconv1") uses no events: the step's gemm16s launch
 * records its own duration on the device (every workgroup takes the constant 100 MHz clock on
 * entry and exit; earliest entry to latest exit), so no packet is added between the launches (an
 * event record costs 4-7 us there and is counted into the bracket).  wt_plan_read_timing waits
 * for the work and returns the summed milliseconds and the number of timed launches since the
 * last reset.  Not thread-safe. */
int wt_plan_num_steps(const wt_plan* p);
int wt_plan_step_name(const wt_plan* p, int32_t index, const char** name);
int wt_plan_set_timing(const wt_plan* p, const char* name_substr);
int wt_plan_read_timing(const wt_plan* p, double* total_ms, int64_t* launches, int32_t reset);

/* Replaces: WavTokenizer.encode_infer (decoder/pretrained.py:186-189) ->
 * EncodecFeatures.infer (decoder/feature_extractors.py:131-142): SEANetEncoder
 * (encoder/modules/seanet.py:143) + ResidualVectorQuantizer.infer (encoder/quantization/vq.py:115-140).
 *   wav      [B][T] fp32 (device)
 *   features [B][512][L] fp32 (device, out) — quantized embedding; may be NULL (a caller that wants the codes alone: the
 *            gather of the codebook rows and the transposed write are then skipped)
 *   codes    [1][B][L] int64 (device, out)
 *   emb_out  optional [B][512][L] fp32: encoder output before quantisation (may be NULL) */
int wt_encode(const wt_plan* p, const float* wav, float* features, int64_t* codes, float* emb_out,
              void* workspace, void* stream);

/* A batch of clips of different lengths on a WT_PLAN_FLAG_MIXED_LENGTH plan (B, Tpad): clip b is lengths[b] samples long and
 * gets exactly the codes and features a plan of its own length computes (the lengths are read on the device, so a recorded
 * graph replays for any lengths).
 *   wav      [B][Tpad] fp32 (device): samples past a clip's length are never read
 *   lengths  [B] int32 (device), each in [wt_plan_min_clip_length(p), Tpad]
 *   features [B][512][Lpad], codes [1][B][Lpad], emb_out (optional) [B][512][Lpad]: past a clip's L = ceil(length / hop) the
 *            codes are -1 and the features (and emb_out) 0.  A clip whose length is outside the range gets -1 codes and NaN
 *            features over its whole row; the other clips and the call's status are not affected.  features may be NULL as in
 *            wt_encode (codes alone).
 * wt_encode refuses a mixed-length plan, and wt_encode_mixed every other plan. */
int wt_encode_mixed(const wt_plan* p, const float* wav, const int32_t* lengths, float* features, int64_t* codes, float* emb_out,
                    void* workspace, void* stream);
/* Replaces: SEANetEncoder (encoder/modules/seanet.py:143) + ResidualVectorQuantizer.encode (encoder/quantization/vq.py:159-168)
 * -> LanguageVectorQuantization.encode (core_vq.py:403-413) on a WT_PLAN_FLAG_RVQ encode plan: per round k < n_q the nearest row
 * of codebook k to the residual (lowest index on ties), r -= that row in fp32.  The codes of n_q = K are the first K rows of
 * n_q = K + 1; row 0 is wt_encode's.
 *   wav   [B][T] fp32 (device);  n_q in [1, num_quantizers] (else WT_ERR_INVALID before any launch);  codes [n_q][B][L] int64 (out)
 * A graph plan's recording is keyed by n_q.  wt_encode refuses a WT_PLAN_FLAG_RVQ plan, and wt_encode_rvq every other plan. */
int wt_encode_rvq(const wt_plan* p, const float* wav, int32_t n_q, int64_t* codes, void* workspace, void* stream);
/* The same on a WT_PLAN_FLAG_RVQ | WT_PLAN_FLAG_MIXED_LENGTH plan (B, Tpad), lengths as in wt_encode_mixed: clip b gets in every
 * one of the n_q rows the codes of a plan of its own length; codes [n_q][B][Lpad] are -1 past a clip's frames and over the whole
 * row of a clip whose length is outside the range. */
int wt_encode_rvq_mixed(const wt_plan* p, const float* wav, const int32_t* lengths, int32_t n_q, int64_t* codes, void* workspace,
                        void* stream);
/* Replaces: ResidualVectorQuantizer.encode (encoder/quantization/vq.py:159-168) on features the caller holds, on a
 * WT_PLAN_QUANTIZE plan (B, L): features [B][512][L] fp32 -> codes [n_q][B][L] int64, the rounds of wt_encode_rvq. */
int wt_quantize(const wt_plan* p, const float* features, int32_t n_q, int64_t* codes, void* workspace, void* stream);
/* The shortest clip a mixed-length plan takes (samples); 0 for any other plan. */
int64_t wt_plan_min_clip_length(const wt_plan* p);
/* SConv1d geometry (encoder/modules/conv.py:54-61, 86-91, 195-211) of a non-causal conv over T samples, the function the plans
 * (and the mixed-length geometry step on the device) use: out = {left pad, total right pad, output frames, reflect length}. */
int wt_sconv_geometry(int64_t T, int32_t k, int32_t stride, int32_t dilation, int32_t out[4]);

/* Replaces: WavTokenizer.codes_to_features (decoder/pretrained.py:209-239).
 *   codes [K][B][L] int64, features [B][512][L] fp32; K <= num_quantizers. */
int wt_codes_to_features(const wt_model* m, const int64_t* codes, int32_t K, int32_t B, int64_t L,
                         float* features, void* stream);

/* Replaces: WavTokenizer.decode (decoder/pretrained.py:192-207): VocosBackbone.forward
 * (decoder/models.py:223-235) + ISTFTHead.forward (decoder/heads.py:42-67) + ISTFT.forward
 * (decoder/spectral_ops.py:33-75).
 *   features [B][512][L] fp32, bandwidth_id in [0, adanorm_num_embeddings), wav_out [B][L*hop] (padding "same";
 *   "center": [B][(L-1)*hop], L >= 2).
 *   backbone_out optional [B][L][dim] fp32 (may be NULL). */
int wt_decode(const wt_plan* p, const float* features, int32_t bandwidth_id, float* wav_out,
              float* backbone_out, void* workspace, void* stream);

/* A batch of clips of different lengths on a WT_PLAN_DECODE_MIXED plan (B, Lpad): clip b is lengths[b] frames long and gets
 * exactly the waveform a WT_PLAN_DECODE plan of its own length computes, whatever the other clips, the padded length and the
 * contents of `features` past its frames (the lengths are read on the device, so a recorded graph replays for any lengths).
 *   features [B][512][Lpad] fp32 (device): frames past a clip's length are read and dropped
 *   lengths  [B] int32 (device), each in [1, Lpad]
 *   wav_out  [B][Lpad*hop] ("center": [B][(Lpad-1)*hop]): clip b's first lengths[b]*hop ("center": (lengths[b]-1)*hop) samples,
 *            zeros behind them.  A length outside the range poisons the whole call: wav_out is NaN and WT_STATUS_BIT_LENGTH is
 *            left in the plan's and the model's status words.
 * The plan runs the shipped split-f16 route only: its creation fails with WT_PLAN_FLAG_UNFUSED, FP32_GEMM, KEEP_STAGES or
 * RANGE_REPORT and with any fp32 range site.  wt_decode refuses a mixed-length plan, and wt_decode_mixed every other plan. */
int wt_decode_mixed(const wt_plan* p, const float* features, const int32_t* lengths, int32_t bandwidth_id, float* wav_out,
                    void* workspace, void* stream);

/* Replaces: WavTokenizer.decode(WavTokenizer.codes_to_features(codes)) (decoder/pretrained.py:192-239) in one call on a
 * WT_PLAN_DECODE_CODES plan (B, L): the bits of wt_codes_to_features followed by wt_decode, without the (B,512,L) feature tensor
 * (the plan's first step gathers the codebook rows, summed over the K codebooks in their order, into the operand of
 * backbone.embed; every later step is the WT_PLAN_DECODE plan's).  The plan takes every flag and range site a WT_PLAN_DECODE
 * plan takes; its creation fails when input_channels differs from the codebook width.
 *   codes [K][B][L] int64 (device), 1 <= K <= num_quantizers (an argument of the call, not of the plan: a recorded graph is
 *   keyed by it); bandwidth_id, wav_out, backbone_out as for wt_decode.
 * A code outside [0, bins) is never used as an index: the frame's row becomes NaN, so that clip's waveform is NaN (the other
 * clips and the call's status are not affected), and wt_model_take_bad_codes reports it once the stream work has completed. */
int wt_decode_codes(const wt_plan* p, const int64_t* codes, int32_t K, int32_t bandwidth_id, float* wav_out,
                    float* backbone_out, void* workspace, void* stream);

/* The same for clips of different lengths on a WT_PLAN_DECODE_CODES_MIXED plan (B, Lpad): clip b is lengths[b] frames long and
 * gets exactly the waveform wt_decode_codes computes for it alone, whatever the other clips, the padded length and the contents
 * of `codes` past its frames (those are never read, range-checked or reported).
 *   codes [K][B][Lpad] int64 (device); lengths, wav_out and the poisoning of a call with a length outside [1, Lpad] as for
 *   wt_decode_mixed.
 * The plan runs the shipped split-f16 route only, like WT_PLAN_DECODE_MIXED (same refusals at creation).  wt_decode_codes refuses
 * a mixed-length plan, and wt_decode_codes_mixed every other plan. */
int wt_decode_codes_mixed(const wt_plan* p, const int64_t* codes, int32_t K, const int32_t* lengths, int32_t bandwidth_id,
                          float* wav_out, void* workspace, void* stream);

/* Replaces: ISTFTHead.forward (decoder/heads.py:42-67) + ISTFT.forward (decoder/spectral_ops.py:33-75) on its own,
 * reached by callers as model.head(x).  x [B][L][dim] fp32 (the backbone output), wav_out [B][L*hop] ("center":
 * [B][(L-1)*hop]). */
int wt_head(const wt_plan* p, const float* x, float* wav_out, void* workspace, void* stream);

/* Replaces: SEANetDecoder.forward (encoder/modules/seanet.py:236-238), reached by callers as
 * model.feature_extractor.encodec.decoder(features).  wav_out [B][1][L*hop]. */
int wt_seanet_decode(const wt_plan* p, const float* features, float* wav_out, void* workspace, void* stream);

/* ---- single-stage entry points (unit parity tests) -------------------------------------------
 * Shipped kernels (what the default plans launch): wt_linear modes 2/3, wt_conv1d_s32, wt_vq_nearest (gemm16s.hip +
 * vq_finalize), wt_resblock (resblock16.hip), WT_PLAN_UNIT_LSTM (lstm_persist.hip / the step kernel).  fp32 twins
 * (gemm.hip, resblock.hip: the WT_PLAN_FLAG_FP32_GEMM path): wt_sconv1d, wt_linear mode 0, wt_vq_nearest_f32,
 * wt_resblock with fp32_chain = 1.  The S32 entry points scale each operand by a per-tensor power of two chosen on
 * the device (the plans' producers write S32 unscaled and report |v| >= 65504 through the status word instead). */

/* Replaces: SConv1d.forward with weight-normed Conv1d (encoder/modules/conv.py:195-211), time-major
 * tensors: x [B][T][Cin] -> y [B][Tout][Cout], w [Cout][k][Cin] (already folded), reflect padding,
 * optional ELU on the input (seanet.py:49,124,136).  Tout = ceil(T/stride).  fp32 MFMA chain (gemm.hip). */
int wt_sconv1d(const float* x, const float* w, const float* bias, float* y, int32_t B, int64_t T,
               int32_t Cin, int32_t Cout, int32_t k, int32_t stride, int32_t dilation, int32_t elu_input,
               void* stream);

/* Replaces: nn.Linear.forward as used by ConvNeXtBlock.pwconv1/2 (decoder/modules.py:52,54): y [M][N] =
 * x [M][K] . w[N][K]^T + bias.  f16x3 = 0: fp32 MFMA chain; 1: removed (round 1's in-loop split kernel); 2: the
 * fp32-equivalent split-f16 arithmetic (x = hi + lo * 2^-11, three f16 MFMAs per product, fp32 accumulation) on
 * pre-split "S32" operands staged by LDS-DMA (gemm16s.hip: the plans' producers write S32 directly; here x and w
 * are split into the workspace first, 4*(M+N)*K bytes, K % 32 == 0); 3: as 2 and y is written in S32 too
 * (N % 32 == 0; every 32 outputs of a row = 128 bytes [32 x f16 hi | 32 x f16 lo], value = hi + lo * 2^-11);
 * 4: as 3 with the exact-erf GELU of decoder/modules.py:53 applied first (pwconv1's epilogue as the decode plan runs it).
 * Modes 2 / 3 need 8 KB more workspace (per-tensor scales; clock stamps of the timing-experiment builds). */
int wt_linear(const float* x, const float* w, const float* bias, float* y, int64_t M, int32_t N, int32_t K,
              int32_t f16x3, void* workspace, void* stream);

/* Conv1d on the S32 split-f16 kernel (gemm16s.hip), time-major x [B][T][Cin] -> y [B][Tout][Cout] fp32,
 * w [Cout][k][Cin]: zero_same = 1: nn.Conv1d(k, padding=(k-1)/2) as in decoder/models.py:29-43,177 (stride 1);
 * zero_same = 0: SConv1d reflect padding (conv.py:195-211).  Cin % 32 == 0; workspace 4*(B*T*Cin + Cout*k*Cin) + 256 bytes. */
int wt_conv1d_s32(const float* x, const float* w, const float* bias, float* y, int32_t B, int64_t T, int32_t Cin,
                  int32_t Cout, int32_t k, int32_t stride, int32_t zero_same, void* workspace, void* stream);

/* Replaces: EuclideanCodebook.quantize (encoder/quantization/core_vq.py:175-183): x [N][D] rows,
 * embed [bins][D]; codes_out [N] int64 = argmax_j -(|x|^2 - 2 x.e_j + |e_j|^2), ties -> lowest j.
 * wt_vq_nearest: the encoder plan's kernels (distances on gemm16s.hip with the per-slab argmax epilogue, then
 * vq_finalize; D % 32 == 0); wt_vq_nearest_f32: the fp32 MFMA chain.  workspace: wt_vq_workspace_bytes(N, D, bins).
 * Both return codes only; wt_vq_probe (below) runs the same launches and also hands out the per-slab candidates of the
 * argmax epilogue and vq_finalize's feature output. */
size_t wt_vq_workspace_bytes(int64_t N, int32_t D, int32_t bins);
int wt_vq_nearest(const float* x, const float* embed, int64_t N, int32_t D, int32_t bins, int64_t* codes_out,
                  void* workspace, void* stream);
int wt_vq_nearest_f32(const float* x, const float* embed, int64_t N, int32_t D, int32_t bins, int64_t* codes_out,
                      void* workspace, void* stream);

/* The vector quantiser as the encoder plan runs it, one launch each through the plans' launchers: row_sumsq (|x|^2, and
 * |e|^2 unless `ee` is given), the distance GEMM with the argmax epilogue (kernel 0: gemm16s.hip on split-f16 operands
 * scaled per tensor as in wt_vq_nearest; kernel 1: the fp32 MFMA chain of gemm.hip) and ONE vq_finalize over B clips of
 * L frames.  x [B*L][D] and embed [bins][D] fp32; ee (optional) [bins]: the |e|^2 table to use as is (the models hold one
 * summed serially on the host); codes [B*L] int64; feat (optional) [B][D][L] = embed[codes] transposed; pval / pidx
 * [B*L][nparts]: the GEMM writes its per-slab (value, index) candidates there (nparts: wt_vq_form, 2 per column tile; a slab
 * without columns reads (-inf, 0x7fffffff)).  Kernel 0 needs bins % 4 == 0 and D % 32 == 0, vq_finalize D % 256 == 0; kernel
 * 1 takes any bins >= 1.  Everything is checked before the first HIP call: a refused problem returns WT_ERR_INVALID and
 * launches nothing.  workspace: wt_vq_workspace_bytes(B * L, D, bins), 256-byte aligned. */
typedef struct {
    int32_t size;                   /* sizeof(wt_vq_desc) */
    int32_t kernel;                 /* 0 gemm16s.hip (split-f16), 1 gemm.hip (fp32) */
    int32_t B, L, D, bins;
    const float* x;
    const float* embed;
    const float* ee;                /* optional */
    int64_t* codes;
    float* feat;                    /* optional */
    float* pval;
    int32_t* pidx;
    uint32_t* status;               /* optional device word (range report of the S32 split) */
} wt_vq_desc;
typedef struct {
    int32_t BM, BN, waves_m, waves_n, grid, ntiles;     /* the distance GEMM: grid < ntiles = persistent, tiles walked */
    int32_t group_m, group_n;                           /* its tile order (row tiles per group; column tiles per block, 0 = all) */
    int32_t nparts;                                     /* candidates per row: (column tiles) x (wave columns) */
    int32_t fin_grid_x, fin_grid_y;                     /* vq_finalize: (32-frame tiles, clips) */
} wt_vq_form;
int wt_vq_probe(const wt_vq_desc* d, wt_vq_form* form, void* workspace, void* stream);

/* One round of residual VQ between two distance GEMMs, the kernel of the WT_PLAN_FLAG_RVQ / WT_PLAN_QUANTIZE plans alone, on
 * caller-owned arrays.  pval / pidx [rows][nparts]: the per-slab (value, index) candidates as the distance GEMM leaves them (the
 * first part that reaches the maximum wins; an index outside [0, bins) gives code 0).  x [rows][D], embed [bins][D] fp32;
 * codes [rows] int64; r [rows][D] = x - embed[code] in fp32 (r may be x); r_s32 (optional) the S32 form of r, the bits of
 * wt_split_probe op 0 on r; xx [rows] = |r|^2, the bits of row_sumsq on r; status (optional): WT_STATUS_BIT_RANGE when a
 * non-NaN |r| >= 65504 is converted.  D % 256 == 0.  Everything is checked before the first HIP call: a refused descriptor
 * returns WT_ERR_INVALID and launches nothing. */
typedef struct {
    int32_t size;                   /* sizeof(wt_vq_residual_desc) */
    int32_t D, bins, nparts;
    int64_t rows;
    const float* pval;
    const int32_t* pidx;
    const float* x;
    const float* embed;
    int64_t* codes;
    float* r;
    void* r_s32;                    /* optional */
    float* xx;
    uint32_t* status;               /* optional device word */
} wt_vq_residual_desc;
typedef struct {
    int32_t grid, block;            /* one wave per row, four rows per workgroup */
    int32_t out_s32;
} wt_vq_residual_form;
int wt_vq_residual_probe(const wt_vq_residual_desc* d, wt_vq_residual_form* form, void* stream);

/* One GEMM launch through the plans' own launchers, with every argument a plan sets: the unit tests' view of each
 * (epilogue, output format) pair and of each tile form the launchers pick.  Operands are fp32 device arrays in the
 * plans' layouts (activations time-major [clip][frame][channel], B operand [N][K] with K = taps * Cin).  engine 0
 * (gemm16s.hip) splits them into the S32 form in the workspace as the plans hold them: a B operand that is a weight
 * (b_is_act = 0) with its per-tensor power-of-two scale and acc_scale, activations (A, A2, a B operand with
 * b_is_act = 1) unscaled (the weight is read back to choose its scale: the call waits for `stream` once); a tap-paired B operand (tap_pair = 1) must already be packed in the paired tap order.
 * engine 1 (gemm.hip) reads the fp32 arrays directly.  engine 2 is engine 0 on the one-product twin of the kernel
 * (WT_PLAN_FLAG_F16_GEMM: same operand split, workspace, checks and tile form; the decode plans' (epi, out) pairs only, no
 * mix_geom).  epi / out / pro take the values of the library's Epi, Out16s,
 * Pro enums (the argmax epilogue is reached through wt_vq_probe instead).  C (and C2) are written in the format
 * `out` names (S32: 128-byte groups [32 x f16 hi | 32 x f16 lo]).  status: optional device word that the S32
 * producers OR WT_STATUS_BIT_RANGE into.  The whole descriptor is checked before any HIP call: a problem the
 * launchers refuse returns WT_ERR_INVALID and touches no memory.  form (optional): the launch the launcher chose.
 * mix_geom (optional, engine 0): the mixed-length launch of a WT_PLAN_FLAG_MIXED_LENGTH plan.  It points at clip 0's
 * {T_in, Tp, T_out} triple of this conv in a device geometry table (wt_geometry_probe; clip stride wt_geom_words.words); the
 * descriptor's extents are then the padded ones, a clip's rows below its T_out gather reflect-about-Tp positions below its
 * T_in, and its rows past T_out gather nothing.  Every clip's T_in must be at most the descriptor's. */
typedef struct {
    int32_t size;                   /* sizeof(wt_gemm_desc) */
    int32_t engine, epi, out, pro, b_is_act;
    int32_t M, N, K;                /* M = clips * T_out */
    int32_t T_in, T_out, Cin, taps, stride, dil, pad_left, pad_mode, Tp;   /* gather; pad_mode 0 zero, 1 reflect */
    int32_t K1, nz, tap_pair, head_kb;
    float alpha;
    int64_t a_bstride, a_rstride, a2_bstride, a2_rstride, w_rstride, c_rstride, r_rstride, zA, zW, zC;   /* elements */
    const float* A;
    const float* A2;                /* K columns [K1, K) (engine 0 only) */
    const float* B;                 /* [N][K] (per z slice: + z * zW) */
    const float* bias;
    const float* R;
    const float* gamma;
    float* C;
    float* C2;
    uint32_t* status;
    const int32_t* mix_geom;        /* optional, last: `size` may also be the struct's size without it (then NULL) */
} wt_gemm_desc;
typedef struct {
    int32_t BM, BN, waves_m, waves_n, stages, ks, prod, staged, bias_cache, G, tiles;   /* G < tiles: persistent grid */
} wt_launch_form;
size_t wt_gemm_probe_workspace_bytes(const wt_gemm_desc* d);
int wt_gemm_probe(const wt_gemm_desc* d, wt_launch_form* form, void* workspace, void* stream);

/* One launch of one non-GEMM kernel through the plans' own launcher (the unit tests' view of GroupNorm, the row norms,
 * softmax, the ISTFT tail, the Cin = 1 / Cout = 1 convs, ConvTranspose1d, the transposes and the two reductions).
 * All arrays are fp32 device arrays in the plans' layouts, activations time-major [clip][frame][channel]; 16-byte
 * aligned (the softmax scores: 4-byte).  Per op (unused fields are ignored):
 *   GN_APPLY   x [B][L][C], p0 gamma [C], p1 beta [C] -> y [B][L][C] (out_s32: S32 rows), y2 scale [B][C], y3 shift [B][C];
 *              groups, eps, flag = swish, p2 = chunk scratch of B * groups * ceil(L / 128) * 2 floats (optional)
 *   GN_STATS   the same without y, flag and out_s32
 *   ROWNORM    x [B][L][C] -> y [B][L][C] (out_s32: S32 rows); mode 0 dwconv k7 p3 + LayerNorm (p0 dw_w [7][C], p1 dw_b [C]),
 *              1 LayerNorm, 2 per-clip affine (p2 in_scale [B][C], p3 in_shift [B][C]) + LayerNorm; p4 out_scale [C],
 *              p5 out_shift [C], eps
 *   SOFTMAX    x scores [n][ld], L valid columns, in place; y (optional): S32 probabilities [n][ld] instead
 *   ISTFT_OLA  x quarter transforms [4][B * L][Kq], p0 window [n_fft], p1 window^2 [n_fft] -> y [B][hop * L] (flag = 1,
 *              "center": [B][hop * (L - 1)])
 *   CONV_FIRST x wav [B][L], p0 w [k][Cout], p1 bias [Cout] -> y [B][L][Cout]
 *   CONV_LAST  x [B][L][C], p0 w [k][C], p1 bias [1] -> y [B][L]; flag = ELU on the input
 *   TRANSPOSE  x [B][L][C] -> y [B][C][L] (out_s32: S32 rows of L)
 *   CONVTR     x [B][L][C], p0 w [k][C][Cout], p1 bias [Cout] -> y [B][L * stride][Cout]; flag = ELU on the input
 *   ROW_SUMSQ  x [n][C] -> y [n]
 *   S32_AMAX   x S32 array of n values -> y: one uint32 word, atomic max of the bit pattern of max |value|
 *   CODE_ROWS  x codes int64 [k][B][L], p0 table [k * n][C] (k codebooks of n bins) -> y [B][L][C] (out_s32: S32 rows): row (b, t)
 *              = sum over the k codebooks of their row codes[.][b][t], in codebook order; a code outside [0, n) gives a NaN
 *              row and sets y2 (optional: one uint32 word the device can write) to 1; C % 4 == 0, C <= 1024
 * lengths (optional; GN_APPLY, GN_STATS, ROWNORM mode 0, SOFTMAX, ISTFT_OLA, TRANSPOSE, CODE_ROWS): device int32 [B] (SOFTMAX: n / L
 * clips of L query rows each; TRANSPOSE: of the C frames; CODE_ROWS: codes past a clip's length are never read).  The op then runs its length-aware launch (the kernels of a WT_PLAN_DECODE_MIXED
 * plan): the extents are the padded ones, clip b's reductions run over its own lengths[b] rows in the order of a call of that
 * length, and its output rows (ISTFT_OLA: samples) past them are zeros.
 * status: optional device word that the S32 producers OR WT_STATUS_BIT_RANGE into (the launch context's status word is
 * set for the call and restored).  The descriptor is checked before any HIP call: whatever the launcher refuses returns
 * WT_ERR_INVALID with its message and touches no memory.  form (optional): the launch the launcher chose. */
enum { WT_OP_GN_APPLY = 0, WT_OP_GN_STATS = 1, WT_OP_ROWNORM = 2, WT_OP_SOFTMAX = 3, WT_OP_ISTFT_OLA = 4, WT_OP_CONV_FIRST = 5,
       WT_OP_CONV_LAST = 6, WT_OP_TRANSPOSE = 7, WT_OP_CONVTR = 8, WT_OP_ROW_SUMSQ = 9, WT_OP_S32_AMAX = 10,
       /* 11 is not assigned and stays refused as unknown: callers written against the ops above probe it as the first op id
          the library does not know, with a descriptor that CODE_ROWS would otherwise take */
       WT_OP_CODE_ROWS = 12 };
/* wt_op_form.kernel */
enum { WT_OPK_GN_TILE = 1, WT_OPK_GN_CHUNK = 2, WT_OPK_GN_STATS = 3, WT_OPK_ROWNORM = 4, WT_OPK_DWCONV_LN = 5,
       WT_OPK_SOFTMAX_REG = 6, WT_OPK_SOFTMAX_RMW = 7, WT_OPK_ISTFT_OLA = 8, WT_OPK_CONV_FIRST = 9, WT_OPK_CONV_LAST32 = 10,
       WT_OPK_CONV_LAST = 11, WT_OPK_TRANSPOSE = 12, WT_OPK_CONVTR = 13, WT_OPK_ROW_SUMSQ = 14, WT_OPK_S32_AMAX = 15,
       /* the length-aware launches (wt_op_desc.lengths) */
       WT_OPK_TRANSPOSE_MIXED = 16, WT_OPK_GN_MIXED = 17, WT_OPK_DWCONV_LN_MIXED = 18, WT_OPK_SOFTMAX_REG_MIXED = 19,
       WT_OPK_SOFTMAX_RMW_MIXED = 20, WT_OPK_ISTFT_OLA_MIXED = 21,
       /* the gather of the decode-from-codes plans and its length-aware twin */
       WT_OPK_CODE_ROWS = 22, WT_OPK_CODE_ROWS_MIXED = 23 };
typedef struct {
    int32_t size;                   /* sizeof(wt_op_desc) */
    int32_t op;
    int32_t B, L, C;                /* clips, frames (rows) per clip, channels */
    int32_t groups, mode, flag, out_s32;
    int32_t ld, k, stride, Cout, n_fft, hop, Kq;
    float eps;
    int64_t n;                      /* SOFTMAX / ROW_SUMSQ rows, S32_AMAX values */
    const void* x;
    const void *p0, *p1, *p2, *p3, *p4, *p5;
    void *y, *y2, *y3;
    uint32_t* status;
    const int32_t* lengths;         /* optional, last: `size` may also be the struct's size without it (then NULL) */
} wt_op_desc;
typedef struct {
    int32_t kernel;                 /* WT_OPK_* */
    int32_t variant;                /* gn_*: APPLY / SWISH template value (gn_mixed: APPLY); rownorm, dwconv_ln, code_rows: NV; softmax_reg: NV4 */
    int32_t variant2;               /* dwconv_ln: R; rownorm: MODE; gn_tile: waves per group; gn_mixed: forms launched (bit 0 slab /
                                       stats kernel, bit 1 chunked pair) */
    int32_t grid_x, grid_y, grid_z, block, lds;     /* gn_chunk: the apply launch */
} wt_op_form;
int wt_op_probe(const wt_op_desc* d, wt_op_form* form, void* stream);

/* Replaces: SEANetResnetBlock.forward (encoder/modules/seanet.py:62-63): y = shortcut(x) + conv1(elu(conv3(elu(x)))),
 * one fused launch, time-major x [B][T][C] -> y [B][T][C], C = 32 or 64; folded weights w3 [C/2][3][C], w1 [C][C/2],
 * ws [C][C].  wav != NULL (C = 32): x is not read; the tile is built from the waveform wav [B][T] through
 * SEANetEncoder.model[0] (seanet.py:107-110; e0_w [7][32], e0_b [32]).  elu_out: y = elu(.);  out_s32: y in the S32
 * encoding;  fp32_chain = 0: resblock16.hip (split-f16 MFMAs, the shipped kernel), 1: resblock.hip. */
int wt_resblock(const float* x, const float* wav, const float* e0_w, const float* e0_b, const float* w3, const float* b3,
                const float* w1, const float* b1, const float* ws, const float* bs, float* y, int32_t B, int64_t T,
                int32_t C, int32_t elu_out, int32_t out_s32, int32_t fp32_chain, void* stream);
/* wt_resblock's shipped stage-1 form: first conv + resblock + ELU + the stage's strided conv (seanet.py:123-127) in one
 * launch.  wd [64][2r][32] (out, tap, in), y_down [B][ceil(T / r)][64] fp32; r in {2, 4}, T >= 1024. */
int wt_resblock_down(const float* wav, const float* e0_w, const float* e0_b, const float* w3, const float* b3, const float* w1,
                     const float* b1, const float* ws, const float* bs, const float* wd, const float* bd, float* y_down,
                     int32_t B, int64_t T, int32_t r, void* stream);

/* One launch of a fused resblock kernel through the plans' own launchers, with the launch it chose reported: wt_resblock
 * (r = 0) and wt_resblock_down (r = 2 or 4: wd, bd set, y = y_down, elu_out / out_s32 ignored) behind one descriptor, the
 * arrays as described there.  status: optional device word that the split-f16 conversions OR WT_STATUS_BIT_RANGE into.
 * mix_T / mix_Tread (optional, both or none; resblock16.hip only): the mixed-length launch of a WT_PLAN_FLAG_MIXED_LENGTH plan:
 * clip 0's length word and readable-length word in a device geometry table (wt_geometry_probe; clip stride
 * wt_geom_words.words).  T is then the padded length (the row stride of x / wav / y, of y_down through ceil(T / r)) and every
 * clip's own length must lie in [1, T] (r != 0: [1024, T]); rows past a clip's length are neither read nor written.
 * The descriptor is checked before any HIP call: whatever a launcher refuses returns WT_ERR_INVALID with its message. */
typedef struct {
    int32_t size;                   /* sizeof(wt_resblock_desc) */
    int32_t B, T, C, r;
    int32_t elu_out, out_s32, fp32_chain;
    const float *x, *wav, *e0_w, *e0_b, *w3, *b3, *w1, *b1, *ws, *bs, *wd, *bd;
    float* y;
    uint32_t* status;
    const int32_t *mix_T, *mix_Tread;
} wt_resblock_desc;
typedef struct {
    int32_t kernel;                 /* 0 resblock16_kernel, 1 resblock16_mixed_kernel, 2 resblock_kernel (fp32 chain) */
    int32_t C, fold, down, fpw;     /* the instantiation: channels, first conv folded in, down-conv stride (0: none), frames per wave */
    int32_t grid, block, lds, tiles;    /* lds: dynamic LDS bytes; grid < tiles: the persistent loop wraps */
} wt_resblock_form;
int wt_resblock_probe(const wt_resblock_desc* d, wt_resblock_form* form, void* stream);

/* The geometry step of a WT_PLAN_FLAG_MIXED_LENGTH encode plan on its own: from lengths (device int32 [B]) the table
 * geom (device int32 [B][words]) of every conv's {T_in, Tp, T_out} along a chain of n_stages encoder stages (k3 conv, 1x1
 * shortcut, down conv of kernel size kd[s] and stride rd[s]) and the final conv of kernel size kf, as a plan of padded length
 * Tpad and shortest clip tmin writes it.  A length outside [tmin, Tpad] gives the geometry of tmin with a readable length 0.
 * wt_geometry_words: the word offsets inside a clip's entry: stage s starts at stage0 + s * stage_words, its three triples at
 * c3, sc and down from there; `final_conv` is the final conv's triple and L the clip's frame count. */
typedef struct {
    int32_t size;                   /* sizeof(wt_geom_desc) */
    int32_t B, tmin, n_stages;
    int32_t kd[8], rd[8];           /* n_stages entries are read; 8 as wt_arch.ratios holds, the table itself takes max_stages (6) */
    int32_t kf;
    int64_t Tpad;
    const int32_t* lengths;
    int32_t* geom;
} wt_geom_desc;
typedef struct {
    int32_t words, valid, T, Tread, stage0, stage_words, c3, sc, down, final_conv, L, max_stages;
} wt_geom_words;
int wt_geometry_words(int32_t n_stages, wt_geom_words* out);
int wt_geometry_probe(const wt_geom_desc* d, void* stream);

/* Runs a WT_PLAN_UNIT_LSTM plan: x, y [B][L][512] fp32 time-major; y = SLSTM(x) (encoder/modules/lstm.py:31-39) with
 * the encoder's LSTM weights of the plan's model. */
int wt_unit_run(const wt_plan* p, const float* x, float* y, void* workspace, void* stream);

/* The recurrence of an SLSTM (encoder/modules/lstm.py:12-39: nn.LSTM(512, 512, num_layers = 2), zero initial state, y = h1 + x)
 * on its own, through the function the plans' LSTM step calls, on one of the three kernels, with the launch reported.
 *   which   0: the encoder's LSTM weights of the model, 1: the SEANetDecoder's (a model that holds one)
 *   kernel  0: lstm_persist_kernel (one launch; B <= 128, L < 65536, a whole 256-CU MI355X: wt_device_info), 1: lstm_step_kernel on
 *           split-f16 MFMAs, 2: lstm_step_kernel on fp32 MFMAs (L + 1 launches each; L <= 65535).  The model's fall-back state
 *           after a lost step barrier (wt_model_persistent_lstm) is not consulted.
 *   xg      [L][B][2048] fp32, time-major: the layer-0 input projection W_ih_l0 x + b_ih_l0 + b_hh_l0 as data, in the packed gate
 *           order of the kernels: gate g (nn.LSTM order i, f, g, o) of hidden unit j is column (j / 4) * 16 + g * 4 + j % 4
 *   x       [B][L][512] fp32, the skip input;  y [B][L][512] fp32 slots: y = h1 + x, elu_out: elu(.), out_s32: in the S32 encoding
 *           (kernel 2 writes fp32 only, as in the plans)
 *   status  optional device word: WT_STATUS_BIT_RANGE (out_s32 and |y| >= 65504), WT_STATUS_BIT_LSTM (a lost step barrier)
 * workspace: wt_lstm_probe_workspace_bytes(d) bytes, 256-byte aligned (0: the descriptor is not one the probe runs).  Arrays are
 * 16-byte aligned.  The descriptor is checked before any HIP call, the model and the device (one attribute query) before any launch
 * or access to device memory.  After a persistent launch the call waits for `stream`: two
 * persistent launches must never share the GPU, and the probe is outside the ordering that wt_encode and the other run entry
 * points keep among themselves, so do not call it beside them. */
typedef struct {
    int32_t size;                   /* sizeof(wt_lstm_desc) */
    int32_t which, kernel;
    int32_t B, L;
    int32_t elu_out, out_s32;
    const float *xg, *x;
    float* y;
    uint32_t* status;
} wt_lstm_desc;
typedef struct {
    int32_t kernel;                 /* as wt_lstm_desc.kernel */
    int32_t small;                  /* persistent: the SMALL instantiation (at most 8 clips per XCD) */
    int32_t Bx;                     /* persistent: clips per XCD */
    int32_t grid_x, grid_y, block, lds;     /* lds: dynamic LDS bytes */
    int32_t launches;               /* kernel launches of the recurrence: 1, or L + 1 */
} wt_lstm_form;
size_t wt_lstm_probe_workspace_bytes(const wt_lstm_desc* d);
int wt_lstm_probe(const wt_model* m, const wt_lstm_desc* d, wt_lstm_form* form, void* workspace, void* stream);

/* The weights as loaded: every device array of a model that a plan can read, by name, read-only.  One walk over the model
 * (packed.cpp model_weights) lists them in a fixed order; `index` runs over [0, count).  Conv weights are "<layer>.w"
 * [cout][k][cin] and "<layer>.b", GEMM weights "<layer>" [rows][cols]; the S32 copy of either is "<layer>.s32" and names the
 * fp32 array it stands for in `of`.
 *   format     0: fp32; 1: S32 (128-byte groups [32 x f16 hi | 32 x f16 lo], value = (hi + lo / 2048) * acc_scale);
 *              2: the LSTM step kernel's f16 lane packing; 3: the persistent LSTM kernel's f16 lane packing
 *   numel      in 4-byte words (an S32 copy has the footprint of its fp32 array; the f16 packings hold two halves per word)
 *   acc_scale  S32: the factor that undoes the copy's power-of-two storage scale (1: stored as it is);  tap_pair  S32: the
 *              copy holds its taps in paired order (q -> (q >> 1) + (q & 1) * stride)
 *   lazy       1: an fp32 array that a packed image does not store and that is rebuilt from its S32 copy (lazy_scale = the
 *              storage scale of that copy) before the first plan on fp32 operands; asking for it here rebuilds it first.
 *              2: an fp32 array that nothing reads after the load (the tap-paired repacking of a down conv): a model made
 *              from a packed image holds no defined values there.  0: stored
 *   archived   1: the pointer is one that the packed image's model section writes.  Always 1: the listing and the section
 *              come from the same walk over the model
 *   alloc      index of the model allocation that starts at `data`, in the order of the packed image's allocation table (-1: the
 *              pointer is no allocation's base) */
typedef struct {
    int32_t size;                   /* sizeof(wt_weight_info), set by the caller */
    int32_t format;
    char name[64], of[64];
    const void* data;
    int64_t numel;
    int32_t ndim;
    int32_t tap_pair;
    int64_t dims[4];
    float acc_scale, lazy_scale;
    int32_t lazy, archived;
    int32_t alloc, reserved;
} wt_weight_info;
int wt_model_weight_count(const wt_model* m);
int wt_model_weight_info(const wt_model* m, int32_t index, wt_weight_info* out);
/* What the distance GEMM of residual VQ round k reads of codebook k, 0 <= k < num_quantizers: its S32 copy ([bins][512], stored
 * with a power-of-two scale of its own; acc_scale undoes it) and its |e|^2 table [bins] fp32, summed serially on the host.  k = 0
 * returns the listed arrays ("vq.embed.s32", "vq.ee"); the tables of k >= 1 are derived state, built from the fp32 codebooks on
 * the device the first time they are asked for (here or by a residual VQ plan), outside the weight listing and the packed image,
 * and freed with the model.  Any output pointer may be NULL. */
int wt_model_codebook_tables(const wt_model* m, int32_t k, const void** s32, const float** ee, float* acc_scale);

/* The format converters under every S32 operand, through the launchers the plans and the loader call, on caller-owned arrays:
 *   op 0  fp32 x[n] -> S32 out (n words), the values multiplied by scale[0] first when `scale` (device) is given
 *   op 1  S32 x (n words) -> fp32 out[n] = (hi + lo / 2048) * inv_scale
 *   op 2  the per-tensor power-of-two scales of the single-stage entry points: bits[0], bits[1] = bit patterns of max |x|, max |b|
 *         over x[n], b[nb]; out[0], out[1] = the scales, out[2] = 1 / (out[0] * out[1])
 * n is a multiple of 32 for ops 0 and 1.  status: optional device word that op 0 ORs WT_STATUS_BIT_RANGE into when a value it
 * converts is beyond the f16 range.  Arrays are 4-byte aligned, device memory; nothing else is touched. */
typedef struct {
    int32_t size;                   /* sizeof(wt_split_desc) */
    int32_t op;
    int64_t n, nb;
    const void *x, *b;
    void* out;
    const float* scale;
    uint32_t* bits;
    float inv_scale;
    uint32_t* status;
} wt_split_desc;
int wt_split_probe(const wt_split_desc* d, void* stream);

/* After wt_codes_to_features, wt_decode_codes or wt_decode_codes_mixed has completed on its stream: 1 if a call since the last
 * query met a code outside [0, bins) (the frames it touched were written as NaN), else 0; the flag is cleared. */
int wt_model_take_bad_codes(const wt_model* m);

/* ---- helpers on either side of the hot path ------------------------------------- */

/* Replaces: convert_audio (encoder/utils.py:79-92) with target_channels = 1: mean over the C (1 or 2) channels, then
 * torchaudio.transforms.Resample(orig_sr, new_sr) (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99; torchaudio
 * is not in this image: restated from its published algorithm, parity unpinned).  wav [B][C][T] -> out [B][T'],
 * T' = wt_resampler_out_length(T) = ceil(new * T / orig).  Equal rates give the plain channel mean. */
typedef struct wt_resampler wt_resampler;
int     wt_resampler_create(int32_t orig_sr, int32_t new_sr, int32_t device, wt_resampler** out);
void    wt_resampler_destroy(wt_resampler* r);
int64_t wt_resampler_out_length(const wt_resampler* r, int64_t T);
int     wt_convert_audio(const wt_resampler* r, const float* wav, int32_t B, int32_t C, int64_t T, float* out, void* stream);

/* Ragged ingest: the way into wt_encode / wt_encode_mixed for a caller that holds raw PCM.  One launch converts B clips of any
 * rate, channel count (1 or 2), layout and sample type (fp32, or int16 scaled by 1 / 32768) into the rows of the fp32 tensor
 * out [B][T_pad], the `wav` operand of wt_encode / wt_encode_mixed: row b holds in its first n_out columns the bits
 * wt_convert_audio gives for clip b alone as planar fp32; columns from n_out on are not written, and nothing outside a clip's
 * n_in samples per channel is read.  Sample (c, t) of a clip is src[c * ch_stride + t * sample_stride] (strides in elements, not
 * negative): planar (C, T) and interleaved (T, C) are both a descriptor.  clips is a HOST array; src and out are device
 * pointers.  The library uploads the descriptors into workspace (device, wt_ingest_workspace_bytes(B) bytes, 8-byte aligned; its
 * content must stay untouched until the launch has run) on `stream`.  Every descriptor is checked before any device call: a null
 * source or resampler, a sample type other than the two, channels other than 1 or 2, n_in < 1, n_out other than
 * wt_resampler_out_length(resampler, n_in), n_out > T_pad, a source pointer not aligned to its sample type, or a resampler of
 * another device than clip 0's returns WT_ERR_INVALID with a message and touches no memory.
 * wt_ingest is a host-side call around its launch: it waits for an event, may allocate pinned memory and enqueues a copy, so it
 * must NOT be called on a stream that is being captured into a graph (call it before the replay, on the replay's stream).
 * Calls on one device are serialised by a lock for the time of the upload.  The two pinned descriptor blocks and their events
 * per device live until the process ends. */
typedef enum { WT_INGEST_F32 = 0, WT_INGEST_I16 = 1 } wt_ingest_dtype;
typedef struct {
    const void* src;                  /* device */
    int32_t dtype;                    /* wt_ingest_dtype */
    int32_t channels;                 /* 1 or 2 */
    int64_t n_in;                     /* samples per channel */
    int64_t ch_stride, sample_stride; /* elements */
    const wt_resampler* resampler;    /* the clip's rate pair (equal rates: the K = 1 copy) */
    int64_t n_out;                    /* wt_resampler_out_length(resampler, n_in) */
} wt_ingest_clip;
size_t wt_ingest_workspace_bytes(int32_t B);
int    wt_ingest(const wt_ingest_clip* clips, int32_t B, int64_t T_pad, float* out, void* workspace, void* stream);

/* Ragged codes out: spans is a device array [B][2] int64 = {L_b, offset_b}; the first L_b codes of row b of codes [1][B][L_pad]
 * (what wt_encode / wt_encode_mixed write) go to out[offset_b + t], out a flat int64 tensor of out_numel elements (device).  A
 * span with L_b outside [0, L_pad] or that does not fit out is skipped whole. */
int wt_codes_unpack(const int64_t* codes, int32_t B, int64_t L_pad, const int64_t* spans, int64_t* out, int64_t out_numel,
                    void* stream);

/* Replaces: save_audio's clamp / rescale (encoder/utils.py:95-103) + the PCM_S 16 conversion of torchaudio.save
 * (infer.py:70): rescale = 0: clamp to [-limit, limit]; 1: scale by min(limit / max|x|, 1) (workspace: 4 bytes);
 * then round-half-even(x * 32768) clipped to int16 (the backend's rounding rule is not pinned by the reference). */
int wt_pcm16(const float* x, int64_t n, float limit, int32_t rescale, int16_t* out, void* workspace, void* stream);

/* Ragged emit, the mirror of wt_ingest: the way out of wt_decode_codes / wt_decode_codes_mixed / wt_decode / wt_decode_mixed for
 * a caller that wants sound files.  One launch converts B rows of fp32 mono audio at the codec rate (rows of those calls'
 * wav_out) each to its own rate, channel count, layout and sample type at its own destination: sample (c, n) of clip b goes to
 * dst[c * ch_stride + n * sample_stride] (strides in elements, not negative), so planar, interleaved and strided destinations
 * are all a descriptor.
 *   WT_EMIT_F32: sample n is the bits wt_convert_audio gives for that clip alone (B = 1, C = 1, T = n_in): the same window, the
 *     same ascending fmaf chain over the same fp32 table, zeros outside [0, n_in).
 *   WT_EMIT_I16: the bits of wt_pcm16(that, limit, rescale = 0): clamp to [-limit, limit], round-half-even of x * 32768 clipped
 *     to int16, in pcm16_kernel's arithmetic (a NaN becomes what it becomes there).  Per-clip rescale needs a reduction over the
 *     resampled clip: that is wt_emit_rescaled (below), two launches instead of one.
 * With channels = 2 both channels receive the same value (convert_audio's expand, encoder/utils.py:85-86).  Nothing past
 * src[n_in - 1] is read (a decode plan leaves zeros or another clip's pitch there), and nothing outside the clip's
 * n_out * channels destination elements is written.  An interleaved stereo frame (ch_stride 1, sample_stride 2, frame-aligned
 * dst) is one store; runs of int16 with sample_stride 1 are stored two samples per 4-byte word wherever a pair shares an aligned
 * word; an equal-rate clip is copied four samples per thread in 16-byte loads and stores where the alignment allows.  clips is a HOST array; src and dst are device pointers.  The library uploads the descriptors into workspace (device,
 * wt_emit_workspace_bytes(B) bytes, 8-byte aligned; its content must stay untouched until the launch has run) on `stream`; up to
 * 64 clips travel in the launch's own argument block instead and leave the workspace untouched (it must be passed all the same).
 * Every descriptor is checked before any device call: a null src, dst or resampler, a sample type other than the two, channels
 * other than 1 or 2, n_in < 1, n_out other than wt_resampler_out_length(resampler, n_in), a negative stride, channels = 2 with
 * ch_stride = 0 and sample_stride < 2 or with sample_stride = 1 and ch_stride < n_out (the channels would overlap), a dst not aligned to its sample type, for WT_EMIT_I16 a
 * limit outside (0, 1], a resampler of another device than clip 0's, or a window beyond the 64 KiB of dynamic LDS returns
 * WT_ERR_INVALID with a message and touches no memory.
 * Like wt_ingest, wt_emit is a host-side call around its launch (it shares wt_ingest's pinned descriptor blocks, their events and
 * their lock): it waits for an event, may allocate pinned memory and enqueues a copy, so it must NOT be called on a stream that
 * is being captured into a graph (call it behind the replay, on the replay's stream). */
typedef enum { WT_EMIT_F32 = 0, WT_EMIT_I16 = 1 } wt_emit_dtype;
typedef struct {
    const float* src;                 /* device: the clip's row, n_in valid samples */
    int64_t n_in;
    const wt_resampler* resampler;    /* codec rate -> the clip's rate (equal rates: the K = 1 copy) */
    int64_t n_out;                    /* wt_resampler_out_length(resampler, n_in) */
    void* dst;                        /* device */
    int32_t dtype;                    /* wt_emit_dtype */
    int32_t channels;                 /* 1 or 2: both channels get the same value */
    int64_t ch_stride, sample_stride; /* elements: sample (c, n) goes to dst[c * ch_stride + n * sample_stride] */
    float limit;                      /* I16 only: clamp to [-limit, limit] first (save_audio, encoder/utils.py:97-102, rescale = False) */
} wt_emit_clip;
size_t wt_emit_workspace_bytes(int32_t B);
int    wt_emit(const wt_emit_clip* clips, int32_t B, void* workspace, void* stream);

/* Rescaling emit: wt_emit with save_audio's rescale = True (encoder/utils.py:95-103) per clip instead of the clamp.  The
 * descriptors are wt_emit's, unchanged, and so are their checks, but `limit` is read and checked for both sample types.  Two
 * launches over wt_emit's grid (behind a one-block launch that zeroes the peaks): the first computes every resampled sample in wt_emit's arithmetic and keeps max |sample| per clip
 * (an integer atomic max on the bits of a non-negative float: the same in any order), the second emits every sample times
 * s = peak > 0 ? min(limit / peak, 1) : 1, one rounded product, in place of the clamp.
 *   WT_EMIT_I16: the bits of wt_pcm16 with rescale = 1 on the clip's WT_EMIT_F32 output (a clip under the limit: s = 1, no clamp);
 *   WT_EMIT_F32: that fp32 output times s.
 * Every store form of wt_emit is kept (interleaved frames, paired int16 runs, the equal-rate copy, any strides), and nothing is
 * read or written that wt_emit would not read or write.  workspace: wt_emit_rescaled_workspace_bytes(B) bytes, 8-byte aligned:
 * the descriptors' place and one 32-bit peak per clip behind it.  A host-side call around its launches like wt_emit. */
size_t wt_emit_rescaled_workspace_bytes(int32_t B);
int    wt_emit_rescaled(const wt_emit_clip* clips, int32_t B, void* workspace, void* stream);

/* ---- per-clip level control: measure, normalise on the way in, scale on the way out ----------------------------------------
 *
 * Ragged level measurement: per clip out[0] = max |x| (exact) and out[1] = sqrt(sum x^2 / n), fp32.  The sum of squares is a
 * binary tree whose shape depends on n alone: chunks of wt_level_chunk samples, a fixed tree inside a chunk, the chunks' partials
 * added pairwise in one fixed order; no float atomics.  A clip has the same bits alone, at any position of any batch and whatever
 * the grid.  Against the exact value the rms errs by at most (3 + ceil(log2 n)) * 2^-24 relative (n rounded squares, a tree of
 * depth ceil(log2 n), one division, one square root).  clips is a HOST array; x and out are device pointers, 4-byte aligned.  Up
 * to 64 descriptors travel in the launches' argument blocks, more go through workspace (device, wt_level_workspace_bytes(B,
 * total_samples) bytes with total_samples >= the sum of the clips' n, 8-byte aligned), which also holds the chunks' partials.
 * B outside [1, 65535], n < 1, a null or misaligned pointer returns WT_ERR_INVALID before any device call.  Two launches. */
typedef struct {
    const float* x;                   /* device: n samples */
    int64_t n;
    float* out;                       /* device [2]: peak, rms */
} wt_level_clip;
int32_t wt_level_chunk(void);
size_t  wt_level_workspace_bytes(int32_t B, int64_t total_samples);
int     wt_level(const wt_level_clip* clips, int32_t B, void* workspace, void* stream);

/* Measure and apply, in place, on the rows of an ingest output rows [B][T_pad] (device): row b has n[b] valid samples (n: a HOST
 * array, each in [1, T_pad]); columns from n[b] on are neither read nor written.  The measurement is the one above, bit for bit.
 *   WT_NORM_PEAK: d = peak + 1e-8f; y = x / d (IEEE division), then y = y * gain only when gain != 1.  With gain = 1 a row has the
 *     bits of torch's fp32 x / (x.abs().max() + 1e-8) (extract_features.py:27-28); gain = 10^(target_db / 20) rounded to fp32 is a
 *     peak target in dB (the data preparation's `norm -3`, decoder/dataset.py:69-70, but AFTER the resampling, not before it).
 *   WT_NORM_RMS:  d = 1e-8f + rms; y = x / d (EncodecModel._encode_frame, encoder/model.py:153-156, on mono audio); gain must be 1.
 * scales[b] (device, fp32) receives the divisor d.  A silent row stays zeros (scale 1e-8).  workspace:
 * wt_normalize_rows_workspace_bytes(B, T_pad) bytes, 8-byte aligned.  Three launches. */
enum { WT_NORM_PEAK = 0, WT_NORM_RMS = 1 };
size_t wt_normalize_rows_workspace_bytes(int32_t B, int64_t T_pad);
int    wt_normalize_rows(float* rows, int32_t B, int64_t T_pad, const int64_t* n, int32_t mode, float gain, float* scales,
                         void* workspace, void* stream);

/* Ragged row scaling: rows[f][0 .. lens[f]) *= scales[f] for f < F, one rounded product per sample: EncodecModel._decode_frame's
 * `out * scale` (encoder/model.py:180-191) on decoded segment rows, in front of wt_overlap_add_ragged (whose weight * frame is then
 * the reference's weight * (frame * scale), both products rounded).  rows (F device pointers), lens (int64) and scales (fp32) are
 * DEVICE arrays; max_len >= every lens[f] sizes the grid.  Nothing is written past rows[f][lens[f] - 1]. */
int wt_scale_rows(float* const* rows, const int64_t* lens, const float* scales, int32_t F, int64_t max_len, void* stream);

/* ---- integrated loudness in LUFS (ITU-R BS.1770-4 / EBU R 128) ----------------------------------------------------------------
 *
 * K-weighting: two cascaded biquads per channel, coefficients computed in double for the integer rate fs:
 *   high shelf: f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196; K = tan(pi f0 / fs), Vh = 10^(G / 20),
 *     Vb = Vh^0.4996667741545416, a0 = 1 + K / Q + K^2; b = [(Vh + Vb K / Q + K^2) / a0, 2 (K^2 - Vh) / a0, (Vh - Vb K / Q + K^2) / a0],
 *     a = [1, 2 (K^2 - 1) / a0, (1 - K / Q + K^2) / a0];
 *   high pass: f0 = 38.13547087602444, Q = 0.5003270373238773; b = [1, -2, 1], a = [1, 2 (K^2 - 1) / (1 + K / Q + K^2),
 *     (1 - K / Q + K^2) / (1 + K / Q + K^2)]  (at 48 kHz the table of BS.1770-4).
 * The filter starts from zero state at sample 0.  Block j covers samples [floor(j fs / 10), floor((j + 4) fs / 10)) in integer
 * arithmetic (400 ms, step 100 ms); only complete blocks count: J = the number of j with floor((j + 4) fs / 10) <= n.  z_j = the sum
 * over the channels (weight 1.0 each) of the mean square of the filtered block, l_j = -0.691 + 10 log10 z_j.  Absolute gate: blocks
 * with l_j > -70; relative threshold G = -0.691 + 10 log10(mean z over those) - 10; integrated loudness L = -0.691 + 10 log10(mean
 * z over the blocks with l_j > -70 and l_j > G).  J = 0 or no block through the gates: L = -inf.
 * The recurrence and every sum run in fp64 on the device, in an order that depends on n and fs alone: a clip has the same bits
 * alone, at any position of any batch and whatever the grid.  Parity with other implementations of the standard is not pinned. */
typedef struct {
    const float* x;                   /* device: channels planes of n samples */
    int64_t n;
    int32_t channels;                 /* 1 or 2 */
    int64_t channel_stride;           /* floats between the planes (>= n; read with 2 channels only) */
    float* out;                       /* device [3]: L, the relative threshold (-inf when L is), the blocks through both gates */
    float* blocks;                    /* device, nullable: receives the J values l_j (the momentary loudness) */
} wt_loudness_clip;
/* Samples per lane of the chunked evaluation (the lengths at which a clip gains a chunk or a wave of 64 chunks). */
int32_t wt_loudness_chunk(void);
/* J of the definition above, on the host (no device call); 0 for n < 1 or a rate outside [8000, 192000]. */
int64_t wt_loudness_blocks(int64_t n, int32_t sample_rate);
/* The K-weighting of the definition above, on the host (no device call): out[0..5) = b0 b1 b2 a1 a2 of the high shelf, out[5..10)
 * the same of the high pass.  A rate outside [8000, 192000] or a null out returns WT_ERR_INVALID. */
int     wt_kweight_coefficients(int32_t sample_rate, double* out);
/* Ragged loudness measurement by the definition above, one rate per call.  clips is a HOST array; x, out and blocks are device
 * pointers, 4-byte aligned.  Up to 64 descriptors travel in the launches' argument blocks, more go through workspace (device,
 * wt_loudness_workspace_bytes(B, total_samples) bytes with total_samples >= the sum of the clips' n * channels, 8-byte aligned),
 * which also holds the chunks' states and partial sums.  B outside [1, 65535], a rate outside [8000, 192000], n < 1, channels other
 * than 1 or 2, a null or misaligned pointer returns WT_ERR_INVALID before any device call.  Four launches. */
size_t  wt_loudness_workspace_bytes(int32_t B, int64_t total_samples);
int     wt_loudness(const wt_loudness_clip* clips, int32_t B, int32_t sample_rate, void* workspace, void* stream);

/* wt_normalize_rows' third measure: rows [B][T_pad] (device, mono), row b has n[b] valid samples (n: a HOST array, each in
 * [1, T_pad]); columns from n[b] on are neither read nor written.  L is row b's integrated loudness by the definition above,
 * rounded to fp32 as wt_loudness reports it; d = fp32(10^((L - target_lufs) / 20)), y = x / d (IEEE division, one rounding per
 * sample), scales[b] = d (device, fp32).  A row with L = -inf (shorter than 400 ms, silent, or all of it under -70) is left as it
 * is, bit for bit, with d = 1.  There is no limiter: a quiet row with one loud click can exceed +-1 after the gain
 * (wt_normalize_rows_lufs_tp below bounds the gain by the row's true peak).  A non-finite
 * target returns WT_ERR_INVALID like the refusals of wt_loudness, before any device call.  workspace:
 * wt_normalize_rows_lufs_workspace_bytes(B, T_pad) bytes, 8-byte aligned.  Five launches. */
size_t wt_normalize_rows_lufs_workspace_bytes(int32_t B, int64_t T_pad);
int    wt_normalize_rows_lufs(float* rows, int32_t B, int64_t T_pad, const int64_t* n, int32_t sample_rate, double target_lufs,
                              float* scales, void* workspace, void* stream);

/* ---- the rest of an EBU R 128 meter: true peak, short-term loudness, loudness range ----------------------------------------------
 *
 * True peak (ITU-R BS.1770-4 Annex 2, by oversampling).  The factor is F = 4 for fs < 96000, 2 for 96000 <= fs < 192000 and 1 at
 * 192000.  The interpolator is a Hann-windowed sinc of 49 taps, h[j] = sinc((j - 24) / F) * 0.5 (1 - cos(2 pi j / 48)) with
 * sinc(t) = sin(pi t) / (pi t), computed in double on the host and rounded to fp32 (h[0] = h[48] = 0).  This is this project's
 * definition: the construction libebur128 uses, not the 48-coefficient table of the standard, and pinned against neither.  Per
 * channel, sample i in [0, n) and phase p in [1, F):  y = sum over k = 0 .. 48 / F - 1 of h[p + F k] * x[i + 24 / F - k], samples
 * outside [0, n) being 0, accumulated in fp32 from 0 with one fmaf per tap, k ascending.  Phase 0 is |x[i]| itself, unfiltered.
 * The true peak is the maximum of |.| over all phases, samples and channels: never below the sample peak, bit for bit; linear
 * (dBTP = 20 log10 of it, -inf for silence).  A maximum is exact in any order: a clip has the same bits alone, at any position of
 * any batch and at any alignment of its pointer.  Against the interpolation in exact arithmetic a value errs by at most
 * (48 / F + 1) * 2^-24 * max_p sum_k |h[p + F k]| * max |x|.  At F = 1 the true peak is the sample peak.
 *
 * Short-term loudness (EBU Tech 3341) on the 100 ms grid of the loudness section: window j covers samples [floor(j fs / 10),
 * floor((j + 30) fs / 10)), 3 s; only complete windows count: S = the number of j with floor((j + 30) fs / 10) <= n = max(J - 26, 0).
 * z_j = the sum over the channels (weight 1.0 each) of the mean square of the K-weighted window, s_j = -0.691 + 10 log10 z_j, no
 * gate.  A window's energy is the sum of its 30 segment sums (100 ms each, the ones the 400 ms blocks are made of, same bits),
 * added in ascending order from the first, ((s0 + s1) + s2) + ... + s29, in fp64, per channel; the quotients by the window's
 * length are then added in channel order.
 *
 * Loudness range (EBU Tech 3342) over the S short-term values on that 100 ms grid (Tech 3342 asks for at least 2 s of overlap;
 * libebur128 steps by 1 s, ffmpeg by 100 ms; parity with either is not pinned).  Absolute gate: s_j > -70.  Relative gate:
 * s_j > -0.691 + 10 log10(mean z over the absolutely gated) - 20.  Of the m energies through both, in ascending order, the ranks
 * lo = ((m - 1) + 5) / 10 and hi = (19 (m - 1) + 10) / 20 (integer division: the nearest-rank 10 % and 95 % points) are selected
 * exactly, whatever S.  LRA = l(z_hi) - l(z_lo) with l(z) = -0.691 + 10 log10 z in double, rounded to fp32.  m = 0 (a clip under
 * 3 s, silent, or all of it under -70): LRA, low and high are NaN.  Sums run over fixed trees in fp64, no float atomics. */
typedef struct {
    const float* x;                   /* device: channels planes of n samples */
    int64_t n;
    int32_t channels;                 /* 1 or 2 */
    int64_t channel_stride;           /* floats between the planes (>= n; read with 2 channels only) */
    float* out;                       /* device [2]: true peak, sample peak (max |x|), both linear */
} wt_true_peak_clip;
/* Samples per workgroup of the true-peak kernel (the lengths at which a clip gains a tile). */
int32_t wt_true_peak_tile(void);
/* Ragged true-peak measurement by the definition above, one rate per call.  clips is a HOST array; x and out are device pointers,
 * 4-byte aligned.  Up to 64 descriptors travel in the launches' argument blocks, more go through workspace (device,
 * wt_true_peak_workspace_bytes(B, total_samples) bytes with total_samples >= the sum of the clips' n * channels, 8-byte aligned),
 * which also holds one pair of maxima per tile.  out[1] has the bits of wt_level's peak.  B outside [1, 65535], a rate outside
 * [8000, 192000], n < 1, channels other than 1 or 2, a null or misaligned pointer returns WT_ERR_INVALID before any device call.
 * Two launches. */
size_t  wt_true_peak_workspace_bytes(int32_t B, int64_t total_samples);
int     wt_true_peak(const wt_true_peak_clip* clips, int32_t B, int32_t sample_rate, void* workspace, void* stream);

typedef struct {
    const float* x;                   /* device: channels planes of n samples */
    int64_t n;
    int32_t channels;                 /* 1 or 2 */
    int64_t channel_stride;           /* floats between the planes (>= n; read with 2 channels only) */
    float* out;                       /* device [9]: L, the relative threshold, the gated blocks (wt_loudness's triple, same bits); LRA,
                                         the low and the high value in LUFS; the count m through the range gates; the maximum
                                         momentary value; the maximum short-term value (-inf without one) */
    float* momentary;                 /* device, nullable: receives the J values l_j */
    float* short_term;                /* device, nullable: receives the S values s_j */
} wt_loudness_range_clip;
/* S of the definition above, on the host (no device call); 0 for n < 1 or a rate outside [8000, 192000]. */
int64_t wt_short_term_blocks(int64_t n, int32_t sample_rate);
/* Ragged measurement of integrated loudness, short-term loudness and loudness range, one rate per call, on one pass of the
 * K-weighting.  Arguments, refusals and descriptor route as wt_loudness; workspace: wt_loudness_range_workspace_bytes(B,
 * total_samples) bytes, 8-byte aligned.  Four launches: the filter's three, then one workgroup per clip for everything else. */
size_t  wt_loudness_range_workspace_bytes(int32_t B, int64_t total_samples);
int     wt_loudness_range(const wt_loudness_range_clip* clips, int32_t B, int32_t sample_rate, void* workspace, void* stream);

/* wt_normalize_rows_lufs under a true-peak ceiling.  For a row with a finite L: d_L = fp32(10^((L - target_lufs) / 20)) as there,
 * d_P = fp32((double)TP / 10^(max_true_peak_db / 20)) with TP the row's true peak by the definition above, d = max(d_L, d_P),
 * y = x / d (IEEE division), scales[b] = d: the result's true peak does not exceed the ceiling (up to the roundings of d, of the
 * division and of the interpolation), and where d_P <= d_L the row has the bits wt_normalize_rows_lufs gives.  A row without a
 * loudness stays as it is with scale 1.  This bounds the gain; it is no sample-wise limiter.  A non-finite target or ceiling
 * returns WT_ERR_INVALID before any device call.  workspace: wt_normalize_rows_lufs_tp_workspace_bytes(B, T_pad) bytes, 8-byte
 * aligned.  Eight launches: the true peak's two, the loudness's four, the ceiling, the gain. */
size_t wt_normalize_rows_lufs_tp_workspace_bytes(int32_t B, int64_t T_pad);
int    wt_normalize_rows_lufs_tp(float* rows, int32_t B, int64_t T_pad, const int64_t* n, int32_t sample_rate, double target_lufs,
                                 double max_true_peak_db, float* scales, void* workspace, void* stream);

/* Replaces: _linear_overlap_add (encoder/utils.py:17-56), bit for bit: frames [n_frames][rows][frame_len] (the last
 * one holds last_len valid samples), weight [frame_len] = the reference's triangle 0.5 - |linspace(0,1,len+2)[1:-1] - 0.5|,
 * out [rows][stride * (n_frames - 1) + last_len]. */
int wt_linear_overlap_add(const float* frames, const float* weight, int32_t n_frames, int64_t rows, int64_t frame_len,
                          int64_t last_len, int64_t stride, float* out, void* stream);

/* Ragged overlap-add: wt_linear_overlap_add for B recordings in one launch, each with its own number of frames, frame length,
 * stride and total length, its frames read where the decode calls left them.  Recording b's frame f is the row rows[f] (rows: a
 * DEVICE array of n_frames device pointers), of which the first len_f = min(frame_len, total - f * stride) samples are the
 * frame: every frame ends at `total` at the latest, so with stride < frame_len several trailing frames are short (the frames
 * EncodecModel.encode cuts, encoder/model.py:139-145).  Nothing is read past rows[f][len_f - 1] (a decode row is longer than its
 * segment, frames(len) * hop >= len, and holds something else there) and nothing is written outside out[0, total).
 *   out[t] = (sum_f weight[t - f * stride] * rows[f][t - f * stride]) / (sum_f weight[t - f * stride])
 * over the frames covering t in ascending f, products and sums rounded separately, one division: the bits of the reference's
 * `out += weight[:len] * frame; sum_weight += weight[:len]; out / sum_weight` (encoder/utils.py:17-56) and of
 * wt_linear_overlap_add on the same frames.  weight is the reference's triangle built on the host (see wt_linear_overlap_add)
 * over the length of the recording's FIRST frame, min(frame_len, total) entries: a recording shorter than frame_len is one
 * frame, and the reference builds its triangle from that frame.  Recordings of one first-frame length may share a table.
 * clips is a HOST array; rows, the pointers it holds, weight and out are device pointers.  The library uploads the descriptors
 * into workspace (device, wt_overlap_add_ragged_workspace_bytes(B) bytes, 8-byte aligned; its content must stay untouched until
 * the launch has run) on `stream`; up to 64 recordings travel in the launch's own argument block instead and leave the workspace
 * untouched (it must be passed all the same).  Every descriptor is checked before any device call: a null rows, weight or out,
 * n_frames, frame_len, stride or total below 1, n_frames other than ceil(total / stride), stride > frame_len with more than one
 * frame (uncovered samples), total > stride * (n_frames - 1) + frame_len (the last frame would not reach the end), or a
 * misaligned pointer returns WT_ERR_INVALID with a message and touches no memory.  The row pointers themselves live on the device
 * and are the caller's to get right.  The launch goes to the calling thread's current device.
 * Like wt_emit, a call with more than 64 recordings is a host-side call around its launch (it shares wt_ingest's pinned
 * descriptor blocks, their events and their lock) and must NOT be made on a stream that is being captured into a graph. */
typedef struct {
    const float* const* rows;         /* device: n_frames device pointers, frame f's row */
    int64_t n_frames;                 /* ceil(total / stride) */
    int64_t frame_len;                /* samples of a full frame */
    int64_t stride;                   /* samples between the starts of two frames */
    int64_t total;                    /* samples of the recording */
    const float* weight;              /* device [min(frame_len, total)] */
    float* out;                       /* device [total] */
} wt_overlap_add_clip;
size_t wt_overlap_add_ragged_workspace_bytes(int32_t B);
int    wt_overlap_add_ragged(const wt_overlap_add_clip* clips, int32_t B, void* workspace, void* stream);

/* ---- evaluation metric: log-mel spectrograms and their L1 distance ---------------------------- */

/* Replaces: MelSpecReconstructionLoss (decoder/loss.py:12-39) with safe_log (decoder/modules.py:194-205), the reference's
 * val/mel_loss (decoder/experiment.py:257-304), as a metric: no gradient.  The transform restates what
 * torchaudio.transforms.MelSpectrogram(sample_rate, n_fft=1024, hop_length, n_mels, center=True, power=1) computes with its
 * defaults (torchaudio is not in this image: restated from its published algorithm, parity unpinned, like the resampler).  For a
 * clip x of T samples: reflect padding by n_fft / 2 on both sides (T > n_fft / 2, as torch.stft demands), F = 1 + T / hop_length
 * frames of n_fft samples, periodic Hann window, magnitudes S of the n_fft / 2 + 1 bins of the real FFT, triangular filters on the
 * HTK mel scale without area normalisation:
 *   all_freqs = linspace(0, sample_rate / 2 (integer division), n_fft / 2 + 1)
 *   m_pts = linspace(0, 2595 log10(1 + (sample_rate / 2) / 700), n_mels + 2),  f_pts = 700 (10^(m_pts / 2595) - 1)
 *   fb[k][m] = max(0, min((all_freqs[k] - f_pts[m]) / (f_pts[m+1] - f_pts[m]), (f_pts[m+2] - all_freqs[k]) / (f_pts[m+2] - f_pts[m+1])))
 *   M[m][f] = sum_k fb[k][m] S[k][f],  L = log(max(M, 1e-7)),  distance = mean over the clip's n_mels * F entries of |L(a) - L(b)|.
 * Window, twiddles and filters are computed in float64 on the host when the handle is made and rounded once; the FFT runs in fp32.
 * A frame's values depend on that frame's n_fft samples alone, and a clip's spectrogram and distance have the same bits alone, in
 * any batch and at any position of it (no float atomics; fixed summation orders that depend on the clip's F alone).
 * n_fft must be 1024, hop_length in 1..1024, n_mels in 1..128, sample_rate >= 2: anything else is refused (WT_ERR_INVALID).
 * The create call puts its tables on `device` and leaves the calling thread's current device as it found it; the spectrogram
 * and distance calls launch on the current device, which must be the handle's. */
typedef struct wt_mel wt_mel;
int     wt_mel_create(int32_t sample_rate, int32_t n_fft, int32_t hop_length, int32_t n_mels, int32_t device, wt_mel** out);
void    wt_mel_destroy(wt_mel* m);
/* 1 + T / hop_length, or -1 when T <= n_fft / 2 (or m is null) */
int64_t wt_mel_frames(const wt_mel* m, int64_t T);
/* Host only, no device needed: the tables a handle of these parameters uploads.  window [n_fft] and fb, dense
 * [n_fft / 2 + 1][n_mels]; either may be null. */
int     wt_mel_tables(int32_t sample_rate, int32_t n_fft, int32_t n_mels, float* window, float* fb);
/* One clip of a launch.  a, b and out are device pointers, fp32; length counts samples (of a, and of b in a distance call).
 *   spectrogram: out [n_mels][F], F = 1 + length / hop_length; b is ignored
 *   distance:    out is one float */
typedef struct {
    const float* a;
    const float* b;
    int64_t length;
    float* out;
} wt_mel_clip;
/* Bytes of the device workspace of a call with B clips whose frame counts add up to total_frames (a spectrogram call may pass
 * total_frames = 0): the descriptors, then one partial sum per frame of a distance call. */
size_t  wt_mel_workspace_bytes(int32_t B, int64_t total_frames);
/* One launch computes the spectrograms of B clips of any lengths (log = 0: M, else L); a distance call is that launch on both
 * signals of every clip, which writes per frame the sum over the filters of |La - Lb| (the same bits L has in a spectrogram call)
 * to the workspace, and a second small launch that adds each clip's partials and divides by n_mels * F.  Nothing outside
 * [0, length) of a or b is read and nothing outside out's n_mels * F (or one) floats and the workspace is written; the content of
 * the workspace before the call does not matter.  clips is a HOST array.  workspace: device, the bytes above, 8-byte aligned, its
 * content untouched until the launches have run.  Up to 64 clips travel in the launches' own argument blocks: the call then makes
 * no host wait and no copy and may be captured into a graph.  More clips go through the pinned descriptor blocks of wt_ingest and
 * wt_emit (their events and their lock): such a call must NOT be made on a stream that is being captured.  Every descriptor is
 * checked before any device call: a null handle, a null a or out, a null b in a distance call, length <= n_fft / 2, a pointer
 * not aligned to 4 bytes, B outside 1..65535, or a handle of another device than the calling thread's current one returns
 * WT_ERR_INVALID with a message and touches no memory. */
int     wt_mel_spectrogram(const wt_mel* m, const wt_mel_clip* clips, int32_t B, int32_t log, void* workspace, void* stream);
int     wt_mel_distance(const wt_mel* m, const wt_mel_clip* clips, int32_t B, void* workspace, void* stream);

/* ---- evaluation metric: short-time objective intelligibility (STOI, ESTOI) -------------------- */

/* Replaces: the per-file CPU loop `stoi(raw.cpu(), pre.cpu(), sr, extended=False)` of the reference's evaluation script
 * (metrics/infer.py:100-105; pystoi).  STOI is Taal, Hendriks, Heusdens & Jensen 2011, ESTOI is Jensen & Taal 2016; pystoi is not in
 * this image, so the measure is restated from the published algorithm and the parity with pystoi is unpinned (tests/stoi_ref.py
 * holds this definition in float64).  For a pair (clean x, processed y) of T samples each at sample_rate, EPS = 2^-52:
 *  1. Both go to 10 kHz (skipped at 10 kHz): p / q = 10000 / sample_rate reduced, fc = 1 / (2 max(p, q)),
 *     L = ceil((60 - 8) / (28.714 fc / 10)), h = kaiser(2 L + 1, 0.1102 (60 - 8.7)) 2 p fc sinc(2 fc t) for t = -L..L, h <- p h / sum(h);
 *     out[n] = sum over the taps k with (n q + L - k) = i p, 0 <= i < T, of h[k] in[i], for n < ceil(T p / q): zero phase, zeros
 *     outside the clip (scipy.signal.resample_poly(in, p, q, window = h / p)).  Rates with max(p, q) <= 441 are accepted (8, 10, 16,
 *     22.05, 24, 32, 44.1, 48 kHz among them).
 *  2. Silent frames leave, decided on x: w = hanning(258)[1:-1]; the K0 candidate frames of 256 samples start at 0, 128, ... < n - 256;
 *     frame f is kept when ||w x_f|| + EPS > 0.01 (max_f ||w x_f|| + EPS) (40 dB).  Both signals are rebuilt by overlap-adding their
 *     kept windowed frames at hop 128; K frames are kept.
 *  3. The rebuilt signals' frames start at 0, 128, ... < len - 256: J = K - 1 frames; frame j is w times rebuilt samples
 *     [128 j, 128 j + 256), zero-padded to 512, real FFT.
 *  4. Fifteen one-third-octave bands from 150 Hz: band i is the square root of the sum of |X|^2 over bins [e_i, e_i+1),
 *     e = 7 9 11 14 17 22 27 34 43 55 69 87 109 138 174 219.
 *  5. One segment per m in 30..J: the 15 x 30 blocks X, Y of frames [m - 30, m).  `row`: per band over the 30 frames.
 *     STOI:  alpha = ||X||_row / (||Y||_row + EPS), Y' = min(alpha Y, X (1 + 10^(15/20))); X and Y' lose their row means and are
 *            divided by (row norm + EPS); d = sum X Y' / (15 segments).
 *     ESTOI: X and Y lose their row means and are divided by (row norm + EPS), then the same per frame over the 15 bands;
 *            d = sum X Y / (30 segments).
 *     J < 30 gives 1e-5 (pystoi's value; there is no warning, it would need a host wait).
 * The tables are computed in float64 on the host and rounded once; everything on the device is fp32 with fixed summation orders
 * and no float atomics: a pair's result has the same bits alone, in any batch and at any position of it.  The create call puts its
 * tables on `device` and leaves the calling thread's current device as it found it; wt_stoi launches on the current device, which
 * must be the handle's. */
typedef struct wt_stoi_handle wt_stoi_handle;
int     wt_stoi_create(int32_t sample_rate, int32_t device, wt_stoi_handle** out);
void    wt_stoi_destroy(wt_stoi_handle* h);
/* ceil(T p / q): the samples a clip of T has at 10 kHz; -1 for a null handle or T < 0 */
int64_t wt_stoi_resampled_length(const wt_stoi_handle* h, int64_t T);
/* Host only, no device needed: what a handle of this rate uploads.  p, q, L; filter [2 L + 1] (ask for L first); window [256];
 * edges [16].  Every pointer may be null.  WT_ERR_INVALID for a rate that is refused. */
int     wt_stoi_tables(int32_t sample_rate, int32_t* p, int32_t* q, int32_t* L, float* filter, float* window, int32_t* edges);
/* One pair of a call: device pointers, fp32; length counts the samples of each of the two signals; out is one float. */
typedef struct {
    const float* clean;
    const float* processed;
    int64_t length;
    float* out;
} wt_stoi_clip;
/* Where a call leaves its stages for tests; every member may be null.  With n_c = wt_stoi_resampled_length(length_c),
 * K0_c = ceil((n_c - 256) / 128), R_c and F_c the sums of n and K0 over the clips before c:
 *   resampled  [2 sum n]: the clean signal of clip c at 10 kHz from 2 R_c, the processed one from 2 R_c + n_c (not written by a
 *              handle of 10 kHz, whose stages read the inputs themselves)
 *   keep       [sum K0]: 1 for a kept candidate frame, else 0, clip c from F_c
 *   counts     [B][2]: (K0, K)
 *   tob        [30 sum K0]: clip c from 30 F_c as [2][15][K0_c] (clean then processed, band, frame); frames j < K - 1 are written
 * An array given here takes the place of the workspace's own, so a call has the same results with and without taps. */
typedef struct {
    float* resampled;
    int32_t* keep;
    int32_t* counts;
    float* tob;
} wt_stoi_taps;
/* Bytes of the device workspace of a call with B clips whose resampled lengths add up to total_resampled and whose candidate-frame
 * counts K0 add up to total_frames; 0 for a null handle or B < 1. */
size_t  wt_stoi_workspace_bytes(const wt_stoi_handle* h, int32_t B, int64_t total_resampled, int64_t total_frames);
/* STOI (extended = 0) or ESTOI of B pairs of any lengths in six launches, each ragged over the clips.  K never comes back to the
 * host: the launches are sized by K0.  Nothing outside [0, length) of the inputs is read and nothing outside the outs, the
 * workspace and the taps is written; the content of the workspace before the call does not matter.  clips is a HOST array.
 * workspace: device, the bytes above, 8-byte aligned, its content untouched until the launches have run.  Up to 32 clips travel in
 * the launches' own argument blocks: the call then makes no host wait and no copy and may be captured into a graph.  More clips go
 * through the pinned descriptor blocks of wt_ingest and wt_emit (their events and their lock): such a call must NOT be made on a
 * stream that is being captured.  Every descriptor is checked before any device call: a null handle, a null clean, processed or
 * out, a length that leaves no candidate frame (256 samples or fewer at 10 kHz), a pointer not aligned to 4 bytes, B outside
 * 1..32767, or a handle of another device than the calling thread's current one returns WT_ERR_INVALID with a message and touches
 * no memory. */
int     wt_stoi(const wt_stoi_handle* h, const wt_stoi_clip* clips, int32_t B, int32_t extended, void* workspace, void* stream,
                const wt_stoi_taps* taps);

/* ---- evaluation metric: multi-resolution STFT distance ---------------------------------------- */

/* The spectral measure codec papers report beside the mel distance (Yamamoto, Song & Kim 2020, Parallel WaveGAN; what
 * auraloss.freq.MultiResolutionSTFTLoss()(x, y) computes with its defaults).  auraloss is not in this image: the measure is restated
 * from the published definition and the parity with auraloss is unpinned (tests/stftd_ref.py holds this definition in float64).
 * For a pair (estimate x, target y) of T samples each and a resolution r = (n_fft, hop, win_length):
 *   X = stft(x) with center = True: reflect padding by n_fft / 2 on both sides (T > n_fft / 2, as torch.stft demands), F = 1 + T / hop
 *   frames of n_fft samples, a periodic Hann window of win_length samples zero-padded to n_fft with (n_fft - win_length) / 2
 *   (integer division) zeros on its left (win_length = 1: the window [1.], as torch.hann_window(1) gives, not the formula's [0.]),
 *   the n_fft / 2 + 1 bins of the real FFT;
 *   |X| = sqrt(max(re^2 + im^2, 1e-7));
 *   sc_r = || |Y| - |X| ||_F / || |Y| ||_F,   mag_r = mean over the bins and frames of | log|Y| - log|X| |;
 *   distance = mean over the resolutions of (sc_r + mag_r).
 * The clamp keeps every logarithm and denominator finite: two silent signals give exactly 0 for every term.  The defaults of the
 * Python surface are the Parallel WaveGAN set: n_fft (1024, 2048, 512), hop (120, 240, 50), win_length (600, 1200, 240).
 * n_fft must be 512, 1024 or 2048, 1 <= hop <= n_fft, 1 <= win_length <= n_fft, 1 to 8 resolutions per handle, and a distance call
 * needs T > max n_fft / 2: anything else is refused (WT_ERR_INVALID).  Windows and twiddles are computed in float64 on the host
 * when the handle is made and rounded once; the FFT runs in fp32, each signal in a transform of its own.  A frame's values depend on
 * that frame's n_fft samples alone, and a pair's result has the same bits alone, in any batch and at any position of it (no float
 * atomics; fixed summation orders that depend on T alone).  The create call puts its tables on `device` and leaves the calling
 * thread's current device as it found it; the calls launch on the current device, which must be the handle's. */
typedef struct wt_stftd wt_stftd;
int     wt_stftd_create(int32_t n_res, const int32_t* n_fft, const int32_t* hop, const int32_t* win_length, int32_t device,
                        wt_stftd** out);
void    wt_stftd_destroy(wt_stftd* h);
/* 1 + T / hop of resolution r, or -1 when T <= n_fft / 2 of that resolution (or h is null, or there is no resolution r) */
int64_t wt_stftd_frames(const wt_stftd* h, int32_t r, int64_t T);
/* Host only, no device needed: the padded window [n_fft] a handle uploads for (n_fft, win_length); window may be null. */
int     wt_stftd_tables(int32_t n_fft, int32_t win_length, float* window);
/* One pair of a call.  estimate, target and out are device pointers, fp32; length counts the samples of each signal.
 *   distance:  out [1 + 2 n_res]: out[0] the distance, out[1 + 2r] = sc_r, out[2 + 2r] = mag_r; out[0] is the fp32 sum of
 *              (sc_r + mag_r) over r in ascending order, divided by n_res
 *   magnitude: out [n_fft / 2 + 1][F], the clamped |X| of `estimate` at one resolution; target is ignored */
typedef struct {
    const float* estimate;
    const float* target;
    int64_t length;
    float* out;
} wt_stftd_clip;
/* Bytes of the device workspace of a call with B pairs; total_frames is the sum over the pairs and over the handle's resolutions of
 * wt_stftd_frames (a magnitude call may pass 0): the descriptors, then three partial sums per frame.  0 for a null handle or B < 1. */
size_t  wt_stftd_workspace_bytes(const wt_stftd* h, int32_t B, int64_t total_frames);
/* wt_stftd_distance: one launch per resolution, ragged over the B pairs (one wave per frame, both signals, three sums over the
 * frame's bins to the workspace), and one small launch that adds each pair's partials.  wt_stftd_magnitude: the launch of resolution
 * r alone, on `estimate`.  Nothing outside [0, length) of the inputs is read and nothing outside out and the workspace is written;
 * the content of the workspace before the call does not matter.  clips is a HOST array.  workspace: device, the bytes above, 8-byte
 * aligned, its content untouched until the launches have run.  Up to 64 pairs travel in the launches' own argument blocks: the call
 * then makes no host wait and no copy and may be captured into a graph.  More go through the pinned descriptor blocks of wt_ingest
 * and wt_emit (their events and their lock): such a call must NOT be made on a stream that is being captured.  Every descriptor is
 * checked before any device call: a null handle, a null estimate or out, a null target in a distance call, length <= n_fft / 2 (the
 * largest of the call's resolutions), a pointer not aligned to 4 bytes, B outside 1..65535, or a handle of another device than the
 * calling thread's current one returns WT_ERR_INVALID with a message and touches no memory. */
int     wt_stftd_distance(const wt_stftd* h, const wt_stftd_clip* clips, int32_t B, void* workspace, void* stream);
int     wt_stftd_magnitude(const wt_stftd* h, int32_t r, const wt_stftd_clip* clips, int32_t B, void* workspace, void* stream);

/* ---- evaluation metric: SI-SDR and SNR ------------------------------------------------------- */

/* The scale-invariant signal-to-distortion ratio (Le Roux, Wisdom, Erdogan & Hershey 2019; torchmetrics'
 * scale_invariant_signal_distortion_ratio) and the plain signal-to-noise ratio (torchmetrics' signal_noise_ratio; the reference's
 * fork scripts compute it by hand in evaluate_audio_quality), both in dB.  torchmetrics is not in this image: parity with it is
 * unpinned (tests/wavedist_ref.py holds this definition in float64).  For a pair (estimate p, target t) of T >= 1 samples, eps = 2^-23:
 *   with zero_mean, each signal first loses its own mean;
 *   SNR    = 10 log10((sum t^2 + eps) / (sum (t - p)^2 + eps));
 *   SI-SDR = 10 log10((sum (alpha t)^2 + eps) / (sum (alpha t - p)^2 + eps)),  alpha = (sum p t + eps) / (sum t^2 + eps).
 * The residual energies are formed sample by sample in a pass that follows the one giving alpha (and that one follows the means):
 * never from the moments sum p^2, sum p t, sum t^2, which in fp32 lose the measure above 60 dB; centred sums use x - mean.  Two
 * silent signals give (0 + eps) / (0 + eps): exactly 0 dB for both.  fp32, no atomics; the passes run over blocks of
 * wt_wavedist_block() samples and the order of every sum depends on T alone: a pair has the same bits alone, in any batch and at
 * any position of it. */
typedef struct {
    const float* estimate;
    const float* target;
    int64_t length;
    float* out;                       /* [2]: SI-SDR, SNR */
} wt_wavedist_clip;
/* Bytes of the device workspace of a call with B pairs whose lengths add up to total_samples; 0 for B < 1. */
size_t  wt_wavedist_workspace_bytes(int32_t B, int64_t total_samples);
/* The samples one workgroup of a pass adds (tests place lengths either side of it). */
int32_t wt_wavedist_block(void);
/* Both measures of B pairs of any lengths: four launches, six with zero_mean, each ragged over the pairs.  The rules of
 * wt_stftd_distance hold for memory, workspace, the 64 descriptors in the argument blocks and graph capture.  Every descriptor is
 * checked before any device call: null clips or workspace, B outside 1..65535, a null estimate, out or target, length < 1 or a
 * pointer not aligned to 4 bytes returns WT_ERR_INVALID with a message and touches no memory. */
int     wt_wavedist(const wt_wavedist_clip* clips, int32_t B, int32_t zero_mean, void* workspace, void* stream);

/* ---- evaluation metric: pitch, periodicity and voiced / unvoiced F1 --------------------------- */

/* The periodicity family of the reference's evaluation (metrics/periodicity.py: calculate_periodicity_metrics, after cargan): a
 * periodicity RMSE, a pitch RMSE in cents over the jointly voiced frames and the F1 of the voiced / unvoiced decision.  The frame
 * grid, the A-weighted loudness gate and the three formulas are the reference's.  The pitch estimator is NOT: the reference runs
 * CREPE, a network whose weights this project cannot carry; here it is YIN (de Cheveigne & Kawahara 2002) on CREPE's frame grid
 * and search range.  Numbers are comparable between runs of this library, not with CREPE-based tables.  tests/pitch_ref.py holds
 * this definition in float64.  Everything is at 16 kHz:
 *   frames: window 1024, hop 160, not centred: n = 1 + (T - 1024) / 160 for T >= 1024 (torchcrepe.predict(pad=False), and the
 *   center=False spectrogram of predict_pitch); frame f is x[160 f .. 160 f + 1023].
 *   YIN per frame: d(lag) = sum over j < 703 of (x[j] - x[j + lag])^2 for lag = 1..321 (703 = 1024 - 321 terms for every lag),
 *   added term by term from the differences, never as an autocorrelation identity; d'(lag) = d(lag) lag / sum over k <= lag of
 *   d(k), 1 where that sum is 0.  The lag: the first in [30, 320] (550 Hz down to 50 Hz) with d' < threshold, d'(lag) <=
 *   d'(lag - 1) and d'(lag) < d'(lag + 1); without one, the smallest lag that attains the minimum of d' over [30, 320].  With
 *   a, b, c = d'(lag - 1), d'(lag), d'(lag + 1) and den = a - 2b + c: off = 0.5 (a - c) / den clamped to +-0.5 (0 for den <= 0),
 *   f0 = 16000 / (lag + off), periodicity = clamp(1 - (b - 0.25 (a - c) off), 0, 1).
 *   loudness gate: S = |rfft(frame * periodic Hann window of 1024)|^2, 513 bins; dB = 10 log10 max(S, 1e-10), floored at the
 *   clip's maximum dB over all frames and bins - 80 (librosa.power_to_db's top_db, per clip); + the A-weighting of the bin's
 *   frequency clipped below at -80 dB (bin 0: -80); - 20 (torchcrepe's REF_DB); the mean over the 513 bins is the frame's
 *   loudness.  A frame with loudness < silence_threshold has its periodicity set to 0.
 *   voicing: a frame with gated periodicity < unvoiced_threshold is unvoiced and its f0 is NaN.
 *   pair (reference y, estimate y^, n frames each): periodicity_loss = sqrt(mean (p^ - p)^2); pitch_loss = sqrt(mean cents^2) over
 *   the frames voiced in both, cents = 1200 (log2 f0 - log2 f0^), NaN without such a frame; f1 = 2 P R / (P + R) with
 *   P = TP / (TP + FP), R = TP / (TP + FN) of the voiced flags, NaN where P or R is 0 / 0 or both are 0.
 * The reference's constants are silence_threshold -60 and unvoiced_threshold 0.21 (CREPE has no threshold of YIN's kind); the
 * Python surface's defaults are threshold 0.15, -60 and 0.5: 0.21 is calibrated for CREPE's confidence, while 1 - d' is about the
 * normalised autocorrelation at the period.  Window, twiddles and A-weighting are computed in float64 on the host when the handle is made
 * and rounded once; the kernels run in fp32, every summation order depends on the clip's length alone and there are no float
 * atomics: a clip or pair has the same bits alone, in any batch and at any position of it.  The create call puts its tables on
 * `device` and leaves the calling thread's current device as it found it; the calls launch on the current device, which must be
 * the handle's. */
typedef struct wt_pitch wt_pitch;
int     wt_pitch_create(int32_t device, wt_pitch** out);
void    wt_pitch_destroy(wt_pitch* h);
/* 1 + (T - 1024) / 160, or 0 for T < 1024 */
int64_t wt_pitch_frames(int64_t T);
/* Host only, no device needed: the window [1024] and the A-weighting in dB [513] a handle uploads; either may be null. */
int     wt_pitch_tables(float* window, float* a_weight);
/* One clip of a track call.  signal, out and taps are device pointers, fp32; length counts the samples (at 16 kHz); with
 * n = wt_pitch_frames(length): out [2][n]: f0 in Hz (NaN: unvoiced), then the gated periodicity; taps, which may be null, [2][n]:
 * the periodicity before the gate, then the loudness in dB. */
typedef struct {
    const float* signal;
    int64_t length;
    float* out;
    float* taps;
} wt_pitch_clip;
/* One pair of a pair call: out [3] = periodicity_loss, pitch_loss, f1. */
typedef struct {
    const float* reference;
    const float* estimate;
    int64_t length;
    float* out;
} wt_pitch_pair;
/* Bytes of the device workspace of a call with B clips or pairs; total_frames is the sum of wt_pitch_frames over them (a pair
 * counts once): the descriptors, ten floats per frame, two per descriptor.  0 for B < 1. */
size_t  wt_pitch_workspace_bytes(int32_t B, int64_t total_frames);
/* wt_pitch_track: four launches, each ragged over the B clips (one wave per frame): YIN, the frames' largest powers, the clips'
 * maxima, the loudness with the gate.  wt_pitch_pairs: the same over both signals of every pair, the tracks left in the
 * workspace, and a launch that reduces each pair.  The rules of wt_stftd_distance hold for memory, workspace, the 64 descriptors
 * in the argument blocks and graph capture.  Every descriptor is checked before any device call: a null handle, clips or
 * workspace, B outside 1..65535, a misaligned workspace, a NaN threshold, a null signal (reference, estimate) or out, length <
 * 1024, a pointer not aligned to 4 bytes, or a handle of another device than the calling thread's current one returns
 * WT_ERR_INVALID with a message and touches no memory. */
int     wt_pitch_track(const wt_pitch* h, const wt_pitch_clip* clips, int32_t B, float threshold, float silence_threshold,
                       float unvoiced_threshold, void* workspace, void* stream);
int     wt_pitch_pairs(const wt_pitch* h, const wt_pitch_pair* pairs, int32_t B, float threshold, float silence_threshold,
                       float unvoiced_threshold, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WAVTOKENIZER_AMD_H */
