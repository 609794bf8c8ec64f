"""ctypes binding of libwavtok_hip.so (see include/wavtokenizer_amd.h).

There is no CPU fallback: if the library is missing or fails to load, importing this
module raises, and every caller of the product path fails loudly.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_float, c_int32, c_int64, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# WAVTOK_HIP_LIB names another build of the same library (A/B timing of two kernel versions); never a fallback
LIB_PATH = os.environ.get("WAVTOK_HIP_LIB") or os.path.join(_HERE, "libwavtok_hip.so")

# every symbol include/wavtokenizer_amd.h declares
EXPORTS = [
    "wt_last_error", "wt_version", "wt_model_create", "wt_model_destroy", "wt_model_export_bytes", "wt_model_export", "wt_packed_info", "wt_packed_verify", "wt_packed_bytes",
    "wt_model_create_packed", "wt_model_hop", "wt_model_weight_bytes",
    "wt_plan_create", "wt_plan_create_ex", "wt_plan_range_sites", "wt_plan_range_report", "wt_model_persistent_lstm", "wt_device_info", "wt_plan_destroy", "wt_plan_workspace_bytes", "wt_plan_frames", "wt_plan_num_launches", "wt_plan_graph_replays",
    "wt_plan_find_buffer", "wt_plan_buffer_info", "wt_plan_buffer_name", "wt_plan_status", "wt_plan_num_steps", "wt_plan_step_name",
    "wt_plan_set_timing", "wt_plan_read_timing", "wt_model_split_ok", "wt_model_status", "wt_model_take_bad_codes", "wt_encode", "wt_codes_to_features",
    "wt_decode", "wt_seanet_decode", "wt_head", "wt_unit_run", "wt_sconv1d", "wt_linear", "wt_conv1d_s32", "wt_vq_workspace_bytes",
    "wt_vq_nearest", "wt_vq_nearest_f32", "wt_resblock", "wt_resblock_down", "wt_gemm_probe_workspace_bytes", "wt_gemm_probe", "wt_op_probe",
    "wt_resampler_create", "wt_resampler_destroy", "wt_resampler_out_length", "wt_convert_audio", "wt_pcm16",
    "wt_linear_overlap_add", "wt_encode_mixed", "wt_plan_min_clip_length", "wt_sconv_geometry", "wt_decode_mixed",
    "wt_resblock_probe", "wt_geometry_words", "wt_geometry_probe", "wt_lstm_probe_workspace_bytes", "wt_lstm_probe",
    "wt_decode_codes", "wt_decode_codes_mixed", "wt_ingest_workspace_bytes", "wt_ingest", "wt_codes_unpack",
    "wt_emit_workspace_bytes", "wt_emit", "wt_vq_probe", "wt_overlap_add_ragged_workspace_bytes", "wt_overlap_add_ragged",
    "wt_model_weight_count", "wt_model_weight_info", "wt_split_probe",
    "wt_encode_rvq", "wt_encode_rvq_mixed", "wt_quantize", "wt_vq_residual_probe", "wt_model_codebook_tables",
    "wt_mel_create", "wt_mel_destroy", "wt_mel_frames", "wt_mel_tables", "wt_mel_workspace_bytes", "wt_mel_spectrogram", "wt_mel_distance",
    "wt_stoi_create", "wt_stoi_destroy", "wt_stoi_resampled_length", "wt_stoi_tables", "wt_stoi_workspace_bytes", "wt_stoi",
    "wt_stftd_create", "wt_stftd_destroy", "wt_stftd_frames", "wt_stftd_tables", "wt_stftd_workspace_bytes", "wt_stftd_distance",
    "wt_stftd_magnitude", "wt_wavedist_workspace_bytes", "wt_wavedist_block", "wt_wavedist",
    "wt_pitch_create", "wt_pitch_destroy", "wt_pitch_frames", "wt_pitch_tables", "wt_pitch_workspace_bytes", "wt_pitch_track", "wt_pitch_pairs",
    "wt_level_chunk", "wt_level_workspace_bytes", "wt_level", "wt_normalize_rows_workspace_bytes", "wt_normalize_rows", "wt_scale_rows",
    "wt_emit_rescaled_workspace_bytes", "wt_emit_rescaled",
    "wt_loudness_chunk", "wt_loudness_blocks", "wt_kweight_coefficients", "wt_loudness_workspace_bytes", "wt_loudness",
    "wt_normalize_rows_lufs_workspace_bytes", "wt_normalize_rows_lufs",
    "wt_true_peak_tile", "wt_true_peak_workspace_bytes", "wt_true_peak", "wt_short_term_blocks", "wt_loudness_range_workspace_bytes",
    "wt_loudness_range", "wt_normalize_rows_lufs_tp_workspace_bytes", "wt_normalize_rows_lufs_tp",
]

WT_PLAN_ENCODE, WT_PLAN_DECODE, WT_PLAN_SEANET_DECODER, WT_PLAN_HEAD, WT_PLAN_UNIT_LSTM = 0, 1, 2, 3, 4
WT_PLAN_DECODE_MIXED = 5
WT_PLAN_DECODE_CODES, WT_PLAN_DECODE_CODES_MIXED = 6, 7
WT_PLAN_QUANTIZE = 8
WT_PLAN_FLAG_KEEP_STAGES = 1
WT_PLAN_FLAG_FP32_GEMM = 2
WT_PLAN_FLAG_F16_GEMM = 128
WT_PLAN_FLAG_STEP_LSTM = 4
WT_PLAN_FLAG_GRAPH = 8
WT_PLAN_FLAG_UNFUSED = 16
WT_PLAN_FLAG_RANGE_REPORT = 32
WT_PLAN_FLAG_MIXED_LENGTH = 64
WT_PLAN_FLAG_RVQ = 256
WT_SITE_ENCODER, WT_SITE_BB_EMBED, WT_SITE_RES0, WT_SITE_RES1, WT_SITE_ATTN, WT_SITE_RES2, WT_SITE_RES3 = 0, 1, 2, 3, 4, 5, 6
WT_SITE_CNX0, WT_SITE_HEAD, WT_SITE_SEANET_DECODER = 7, 40, 41
WT_ERR_INVALID = -1
WT_ERR_RANGE, WT_ERR_LSTM_SYNC, WT_ERR_INDEX = -6, -7, -8
WT_STATUS_BIT_LSTM, WT_STATUS_BIT_RANGE, WT_STATUS_BIT_LENGTH = 1, 2, 4
BUF_S32, BUF_ELU = 1, 2


class WtArch(ctypes.Structure):
    _fields_ = [("n_ratios", c_int32), ("ratios", c_int32 * 8), ("vq_bins", c_int32), ("num_quantizers", c_int32),
                ("input_channels", c_int32), ("dim", c_int32), ("intermediate_dim", c_int32),
                ("num_layers", c_int32), ("adanorm_num_embeddings", c_int32), ("n_fft", c_int32),
                ("hop_length", c_int32), ("padding_same", c_int32)]


class WtTensor(ctypes.Structure):
    _fields_ = [("name", c_char_p), ("data", POINTER(c_float)), ("numel", c_int64)]


class WtGemmDesc(ctypes.Structure):
    """wt_gemm_desc: one GEMM launch through the plans' launchers (wt_gemm_probe)."""
    _fields_ = ([("size", c_int32), ("engine", c_int32), ("epi", c_int32), ("out", c_int32), ("pro", c_int32), ("b_is_act", c_int32),
                 ("M", c_int32), ("N", c_int32), ("K", c_int32)]
                + [(n, c_int32) for n in ("T_in", "T_out", "Cin", "taps", "stride", "dil", "pad_left", "pad_mode", "Tp",
                                         "K1", "nz", "tap_pair", "head_kb")]
                + [("alpha", c_float)]
                + [(n, c_int64) for n in ("a_bstride", "a_rstride", "a2_bstride", "a2_rstride", "w_rstride", "c_rstride",
                                         "r_rstride", "zA", "zW", "zC")]
                + [(n, c_void_p) for n in ("A", "A2", "B", "bias", "R", "gamma", "C", "C2", "status", "mix_geom")])


class WtLaunchForm(ctypes.Structure):
    _fields_ = [(n, c_int32) for n in ("BM", "BN", "waves_m", "waves_n", "stages", "ks", "prod", "staged", "bias_cache", "G", "tiles")]


WT_OP_GN_APPLY, WT_OP_GN_STATS, WT_OP_ROWNORM, WT_OP_SOFTMAX, WT_OP_ISTFT_OLA, WT_OP_CONV_FIRST = 0, 1, 2, 3, 4, 5
WT_OP_CONV_LAST, WT_OP_TRANSPOSE, WT_OP_CONVTR, WT_OP_ROW_SUMSQ, WT_OP_S32_AMAX = 6, 7, 8, 9, 10
WT_OP_CODE_ROWS = 12             # (11 is unassigned: the library refuses it as unknown)
WT_OPK_NAMES = {1: "gn_tile", 2: "gn_chunk", 3: "gn_stats", 4: "rownorm", 5: "dwconv_ln", 6: "softmax_reg", 7: "softmax_rmw",
                8: "istft_ola", 9: "conv_first", 10: "conv_last32", 11: "conv_last", 12: "transpose", 13: "convtr",
                14: "row_sumsq", 15: "s32_amax", 16: "transpose_mixed", 17: "gn_mixed", 18: "dwconv_ln_mixed",
                19: "softmax_reg_mixed", 20: "softmax_rmw_mixed", 21: "istft_ola_mixed", 22: "code_rows", 23: "code_rows_mixed"}
WT_OPK_CODE_ROWS, WT_OPK_CODE_ROWS_MIXED = 22, 23


class WtOpDesc(ctypes.Structure):
    """wt_op_desc: one launch of one non-GEMM kernel through the plans' launcher (wt_op_probe)."""
    _fields_ = ([(n, c_int32) for n in ("size", "op", "B", "L", "C", "groups", "mode", "flag", "out_s32", "ld", "k", "stride",
                                        "Cout", "n_fft", "hop", "Kq")]
                + [("eps", c_float), ("n", c_int64)]
                + [(n, c_void_p) for n in ("x", "p0", "p1", "p2", "p3", "p4", "p5", "y", "y2", "y3", "status", "lengths")])


class WtOpForm(ctypes.Structure):
    _fields_ = [(n, c_int32) for n in ("kernel", "variant", "variant2", "grid_x", "grid_y", "grid_z", "block", "lds")]


class WtResblockDesc(ctypes.Structure):
    """wt_resblock_desc: one fused resblock launch through the plans' launchers (wt_resblock_probe)."""
    _fields_ = ([(n, c_int32) for n in ("size", "B", "T", "C", "r", "elu_out", "out_s32", "fp32_chain")]
                + [(n, c_void_p) for n in ("x", "wav", "e0_w", "e0_b", "w3", "b3", "w1", "b1", "ws", "bs", "wd", "bd", "y", "status",
                                          "mix_T", "mix_Tread")])


class WtResblockForm(ctypes.Structure):
    _fields_ = [(n, c_int32) for n in ("kernel", "C", "fold", "down", "fpw", "grid", "block", "lds", "tiles")]


class WtVqDesc(ctypes.Structure):
    """wt_vq_desc: the encoder plan's VQ launches on caller-owned arrays (wt_vq_probe)."""
    _fields_ = ([(n, c_int32) for n in ("size", "kernel", "B", "L", "D", "bins")]
                + [(n, c_void_p) for n in ("x", "embed", "ee", "codes", "feat", "pval", "pidx", "status")])


class WtVqForm(ctypes.Structure):
    _fields_ = [(n, c_int32) for n in ("BM", "BN", "waves_m", "waves_n", "grid", "ntiles", "group_m", "group_n", "nparts",
                                       "fin_grid_x", "fin_grid_y")]


class WtVqResidualDesc(ctypes.Structure):
    """wt_vq_residual_desc: one residual VQ round's kernel on caller-owned arrays (wt_vq_residual_probe)."""
    _fields_ = ([(n, c_int32) for n in ("size", "D", "bins", "nparts")] + [("rows", c_int64)]
                + [(n, c_void_p) for n in ("pval", "pidx", "x", "embed", "codes", "r", "r_s32", "xx", "status")])


class WtVqResidualForm(ctypes.Structure):
    _fields_ = [(n, c_int32) for n in ("grid", "block", "out_s32")]


LSTM_PERSIST, LSTM_STEP_F16, LSTM_STEP_F32 = 0, 1, 2


class WtLstmDesc(ctypes.Structure):
    """wt_lstm_desc: the recurrence of an SLSTM on one of its kernels, as the plans issue it (wt_lstm_probe)."""
    _fields_ = ([(n, c_int32) for n in ("size", "which", "kernel", "B", "L", "elu_out", "out_s32")]
                + [(n, c_void_p) for n in ("xg", "x", "y", "status")])


class WtLstmForm(ctypes.Structure):
    _fields_ = [(n, c_int32) for n in ("kernel", "small", "Bx", "grid_x", "grid_y", "block", "lds", "launches")]


class WtGeomDesc(ctypes.Structure):
    """wt_geom_desc: the geometry step of a mixed-length encode plan on its own (wt_geometry_probe)."""
    _fields_ = [("size", c_int32), ("B", c_int32), ("tmin", c_int32), ("n_stages", c_int32), ("kd", c_int32 * 8), ("rd", c_int32 * 8),
                ("kf", c_int32), ("Tpad", c_int64), ("lengths", c_void_p), ("geom", c_void_p)]


class WtGeomWords(ctypes.Structure):
    _fields_ = [(n, c_int32) for n in ("words", "valid", "T", "Tread", "stage0", "stage_words", "c3", "sc", "down", "final_conv",
                                       "L", "max_stages")]


WT_INGEST_F32, WT_INGEST_I16 = 0, 1


class WtIngestClip(ctypes.Structure):
    """wt_ingest_clip: one clip of a ragged ingest launch (wt_ingest)."""
    _fields_ = [("src", c_void_p), ("dtype", c_int32), ("channels", c_int32), ("n_in", c_int64), ("ch_stride", c_int64),
                ("sample_stride", c_int64), ("resampler", c_void_p), ("n_out", c_int64)]


WT_EMIT_F32, WT_EMIT_I16 = 0, 1


class WtEmitClip(ctypes.Structure):
    """wt_emit_clip: one clip of a ragged emit launch (wt_emit)."""
    _fields_ = [("src", c_void_p), ("n_in", c_int64), ("resampler", c_void_p), ("n_out", c_int64), ("dst", c_void_p),
                ("dtype", c_int32), ("channels", c_int32), ("ch_stride", c_int64), ("sample_stride", c_int64), ("limit", c_float)]


WT_NORM_PEAK, WT_NORM_RMS = 0, 1
WT_NORM_LUFS = 2                 # (Python side only: audio.normalize_rows routes it to wt_normalize_rows_lufs)


class WtLevelClip(ctypes.Structure):
    """wt_level_clip: one clip of a level measurement (wt_level)."""
    _fields_ = [("x", c_void_p), ("n", c_int64), ("out", c_void_p)]


class WtLoudnessClip(ctypes.Structure):
    """wt_loudness_clip: one clip of a loudness measurement (wt_loudness)."""
    _fields_ = [("x", c_void_p), ("n", c_int64), ("channels", c_int32), ("channel_stride", c_int64), ("out", c_void_p),
                ("blocks", c_void_p)]


class WtTruePeakClip(ctypes.Structure):
    """wt_true_peak_clip: one clip of a true-peak measurement (wt_true_peak)."""
    _fields_ = [("x", c_void_p), ("n", c_int64), ("channels", c_int32), ("channel_stride", c_int64), ("out", c_void_p)]


class WtLoudnessRangeClip(ctypes.Structure):
    """wt_loudness_range_clip: one clip of a loudness-range measurement (wt_loudness_range)."""
    _fields_ = [("x", c_void_p), ("n", c_int64), ("channels", c_int32), ("channel_stride", c_int64), ("out", c_void_p),
                ("momentary", c_void_p), ("short_term", c_void_p)]


class WtOverlapAddClip(ctypes.Structure):
    """wt_overlap_add_clip: one recording of a ragged overlap-add launch (wt_overlap_add_ragged)."""
    _fields_ = [("rows", c_void_p), ("n_frames", c_int64), ("frame_len", c_int64), ("stride", c_int64), ("total", c_int64),
                ("weight", c_void_p), ("out", c_void_p)]


class WtMelClip(ctypes.Structure):
    """wt_mel_clip: one clip of a mel launch (wt_mel_spectrogram, wt_mel_distance)."""
    _fields_ = [("a", c_void_p), ("b", c_void_p), ("length", c_int64), ("out", c_void_p)]


class WtStoiClip(ctypes.Structure):
    """wt_stoi_clip: one pair of a STOI call (wt_stoi)."""
    _fields_ = [("clean", c_void_p), ("processed", c_void_p), ("length", c_int64), ("out", c_void_p)]


class WtStftdClip(ctypes.Structure):
    """wt_stftd_clip: one pair of an STFT-distance call (wt_stftd_distance, wt_stftd_magnitude)."""
    _fields_ = [("estimate", c_void_p), ("target", c_void_p), ("length", c_int64), ("out", c_void_p)]


class WtWavedistClip(ctypes.Structure):
    """wt_wavedist_clip: one pair of a time-domain call (wt_wavedist)."""
    _fields_ = [("estimate", c_void_p), ("target", c_void_p), ("length", c_int64), ("out", c_void_p)]


class WtPitchClip(ctypes.Structure):
    """wt_pitch_clip: one clip of a pitch-track call (wt_pitch_track)."""
    _fields_ = [("signal", c_void_p), ("length", c_int64), ("out", c_void_p), ("taps", c_void_p)]


class WtPitchPair(ctypes.Structure):
    """wt_pitch_pair: one pair of a periodicity-metrics call (wt_pitch_pairs)."""
    _fields_ = [("reference", c_void_p), ("estimate", c_void_p), ("length", c_int64), ("out", c_void_p)]


class WtStoiTaps(ctypes.Structure):
    """wt_stoi_taps: where wt_stoi leaves its stages for tests."""
    _fields_ = [("resampled", c_void_p), ("keep", c_void_p), ("counts", c_void_p), ("tob", c_void_p)]


WT_WEIGHT_F32, WT_WEIGHT_S32, WT_WEIGHT_LSTM_F16, WT_WEIGHT_LSTM_PERSIST = 0, 1, 2, 3
WT_SPLIT, WT_UNSPLIT, WT_POW2_SCALES = 0, 1, 2


class WtWeightInfo(ctypes.Structure):
    """wt_weight_info: one device array of a model as loaded (wt_model_weight_info)."""
    _fields_ = [("size", c_int32), ("format", c_int32), ("name", ctypes.c_char * 64), ("of", ctypes.c_char * 64), ("data", c_void_p),
                ("numel", c_int64), ("ndim", c_int32), ("tap_pair", c_int32), ("dims", c_int64 * 4), ("acc_scale", c_float),
                ("lazy_scale", c_float), ("lazy", c_int32), ("archived", c_int32), ("alloc", c_int32), ("reserved", c_int32)]


class WtSplitDesc(ctypes.Structure):
    """wt_split_desc: one launch of a format converter under the S32 operands (wt_split_probe)."""
    _fields_ = [("size", c_int32), ("op", c_int32), ("n", c_int64), ("nb", c_int64), ("x", c_void_p), ("b", c_void_p),
                ("out", c_void_p), ("scale", c_void_p), ("bits", c_void_p), ("inv_scale", c_float), ("status", c_void_p)]


class WavTokError(RuntimeError):
    def __init__(self, msg, status=0):
        super().__init__(msg)
        self.status = status


def _load() -> ctypes.CDLL:
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()' "
            "or make -C wavtokenizer_amd/csrc). There is no CPU fallback for the product path.")
    lib = ctypes.CDLL(LIB_PATH)
    if os.environ.get("WAVTOK_HIP_LIB"):
        # A/B timing against an older build of the library (tools/build_prev.sh): entry points it does not have yet are
        # replaced by a stub that fails when called, so that the timing tools can still bind the ones they use
        class _Missing:
            def __init__(self, name):
                self.name, self.argtypes, self.restype = name, None, None

            def __call__(self, *a):
                raise WavTokError(f"{LIB_PATH} has no {self.name}")
        for sym in EXPORTS:
            try:
                getattr(lib, sym)
            except AttributeError:
                setattr(lib, sym, _Missing(sym))
    lib.wt_last_error.restype = c_char_p
    lib.wt_version.restype = c_char_p
    lib.wt_model_create.argtypes = [POINTER(WtArch), POINTER(WtTensor), c_int32, c_int32, POINTER(c_void_p)]
    lib.wt_model_destroy.argtypes = [c_void_p]
    lib.wt_model_destroy.restype = None
    lib.wt_model_export_bytes.argtypes = [c_void_p]
    lib.wt_model_export_bytes.restype = c_size_t
    lib.wt_model_export.argtypes = [c_void_p, c_void_p, c_size_t]
    lib.wt_packed_info.argtypes = [c_void_p, c_size_t, POINTER(WtArch), POINTER(c_int32), POINTER(ctypes.c_uint64)]
    lib.wt_packed_verify.argtypes = [c_void_p, c_size_t]
    lib.wt_packed_bytes.argtypes = [c_void_p, c_size_t]
    lib.wt_packed_bytes.restype = c_size_t
    lib.wt_model_create_packed.argtypes = [c_void_p, c_size_t, c_int32, POINTER(c_void_p)]
    lib.wt_model_hop.argtypes = [c_void_p]
    lib.wt_model_weight_bytes.argtypes = [c_void_p]
    lib.wt_model_weight_bytes.restype = c_int64
    lib.wt_plan_create.argtypes = [c_void_p, c_int32, c_int32, c_int64, c_int32, POINTER(c_void_p)]
    lib.wt_plan_create_ex.argtypes = [c_void_p, c_int32, c_int32, c_int64, c_int32, ctypes.c_uint64, POINTER(c_void_p)]
    lib.wt_plan_range_sites.argtypes = [c_void_p, POINTER(ctypes.c_uint64), c_int32]
    lib.wt_plan_range_report.argtypes = [c_void_p, c_int32, POINTER(c_char_p), POINTER(c_char_p), POINTER(c_float)]
    lib.wt_model_persistent_lstm.argtypes = [c_void_p]
    lib.wt_device_info.argtypes = [c_int32, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32)]
    lib.wt_plan_destroy.argtypes = [c_void_p]
    lib.wt_plan_destroy.restype = None
    lib.wt_plan_workspace_bytes.argtypes = [c_void_p]
    lib.wt_plan_workspace_bytes.restype = c_size_t
    lib.wt_plan_frames.argtypes = [c_void_p]
    lib.wt_plan_frames.restype = c_int64
    lib.wt_plan_num_launches.argtypes = [c_void_p]
    lib.wt_plan_graph_replays.argtypes = [c_void_p]
    lib.wt_plan_graph_replays.restype = c_int64
    lib.wt_plan_find_buffer.argtypes = [c_void_p, c_char_p, POINTER(c_size_t), POINTER(c_size_t)]
    lib.wt_plan_buffer_info.argtypes = [c_void_p, c_char_p, POINTER(c_size_t), POINTER(c_size_t), POINTER(c_int32)]
    lib.wt_plan_status.argtypes = [c_void_p, POINTER(c_int32), c_int32]
    lib.wt_model_split_ok.argtypes = [c_void_p]
    lib.wt_model_status.argtypes = [c_void_p, POINTER(c_int32), c_int32]
    lib.wt_model_take_bad_codes.argtypes = [c_void_p]
    lib.wt_unit_run.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.wt_plan_buffer_name.argtypes = [c_void_p, c_int32, POINTER(c_char_p)]
    lib.wt_plan_num_steps.argtypes = [c_void_p]
    lib.wt_plan_step_name.argtypes = [c_void_p, c_int32, POINTER(c_char_p)]
    lib.wt_plan_set_timing.argtypes = [c_void_p, c_char_p]
    lib.wt_plan_read_timing.argtypes = [c_void_p, POINTER(ctypes.c_double), POINTER(c_int64), c_int32]
    lib.wt_encode.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.wt_encode_mixed.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.wt_decode_mixed.argtypes = [c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]
    lib.wt_decode_codes.argtypes = [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.wt_decode_codes_mixed.argtypes = [c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]
    lib.wt_plan_min_clip_length.argtypes = [c_void_p]
    lib.wt_plan_min_clip_length.restype = c_int64
    lib.wt_sconv_geometry.argtypes = [c_int64, c_int32, c_int32, c_int32, POINTER(c_int32)]
    lib.wt_codes_to_features.argtypes = [c_void_p, c_void_p, c_int32, c_int32, c_int64, c_void_p, c_void_p]
    lib.wt_decode.argtypes = [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.wt_seanet_decode.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.wt_head.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.wt_sconv1d.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_int32, c_int32, c_int32,
                               c_int32, c_int32, c_int32, c_void_p]
    lib.wt_linear.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_int32, c_void_p, c_void_p]
    lib.wt_conv1d_s32.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_int32, c_int32, c_int32,
                                  c_int32, c_int32, c_void_p, c_void_p]
    lib.wt_vq_workspace_bytes.argtypes = [c_int64, c_int32, c_int32]
    lib.wt_vq_workspace_bytes.restype = c_size_t
    lib.wt_vq_nearest.argtypes = [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p]
    lib.wt_vq_nearest_f32.argtypes = [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p]
    lib.wt_resblock.argtypes = [c_void_p] * 11 + [c_int32, c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p]
    lib.wt_resblock_down.argtypes = [c_void_p] * 12 + [c_int32, c_int64, c_int32, c_void_p]
    lib.wt_gemm_probe_workspace_bytes.argtypes = [POINTER(WtGemmDesc)]
    lib.wt_gemm_probe_workspace_bytes.restype = c_size_t
    lib.wt_gemm_probe.argtypes = [POINTER(WtGemmDesc), POINTER(WtLaunchForm), c_void_p, c_void_p]
    lib.wt_op_probe.argtypes = [POINTER(WtOpDesc), POINTER(WtOpForm), c_void_p]
    lib.wt_resblock_probe.argtypes = [POINTER(WtResblockDesc), POINTER(WtResblockForm), c_void_p]
    lib.wt_vq_probe.argtypes = [POINTER(WtVqDesc), POINTER(WtVqForm), c_void_p, c_void_p]
    lib.wt_lstm_probe_workspace_bytes.argtypes = [POINTER(WtLstmDesc)]
    lib.wt_lstm_probe_workspace_bytes.restype = c_size_t
    lib.wt_lstm_probe.argtypes = [c_void_p, POINTER(WtLstmDesc), POINTER(WtLstmForm), c_void_p, c_void_p]
    lib.wt_geometry_words.argtypes = [c_int32, POINTER(WtGeomWords)]
    lib.wt_geometry_probe.argtypes = [POINTER(WtGeomDesc), c_void_p]
    lib.wt_resampler_create.argtypes = [c_int32, c_int32, c_int32, POINTER(c_void_p)]
    lib.wt_resampler_destroy.argtypes = [c_void_p]
    lib.wt_resampler_destroy.restype = None
    lib.wt_resampler_out_length.argtypes = [c_void_p, c_int64]
    lib.wt_resampler_out_length.restype = c_int64
    lib.wt_convert_audio.argtypes = [c_void_p, c_void_p, c_int32, c_int32, c_int64, c_void_p, c_void_p]
    lib.wt_pcm16.argtypes = [c_void_p, c_int64, ctypes.c_float, c_int32, c_void_p, c_void_p, c_void_p]
    lib.wt_linear_overlap_add.argtypes = [c_void_p, c_void_p, c_int32, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p]
    lib.wt_ingest_workspace_bytes.argtypes = [c_int32]
    lib.wt_ingest_workspace_bytes.restype = c_size_t
    lib.wt_ingest.argtypes = [POINTER(WtIngestClip), c_int32, c_int64, c_void_p, c_void_p, c_void_p]
    lib.wt_codes_unpack.argtypes = [c_void_p, c_int32, c_int64, c_void_p, c_void_p, c_int64, c_void_p]
    lib.wt_emit_workspace_bytes.argtypes = [c_int32]
    lib.wt_emit_workspace_bytes.restype = c_size_t
    lib.wt_emit.argtypes = [POINTER(WtEmitClip), c_int32, c_void_p, c_void_p]
    lib.wt_overlap_add_ragged_workspace_bytes.argtypes = [c_int32]
    lib.wt_overlap_add_ragged_workspace_bytes.restype = c_size_t
    lib.wt_overlap_add_ragged.argtypes = [POINTER(WtOverlapAddClip), c_int32, c_void_p, c_void_p]
    lib.wt_model_weight_count.argtypes = [c_void_p]
    lib.wt_model_weight_info.argtypes = [c_void_p, c_int32, POINTER(WtWeightInfo)]
    lib.wt_split_probe.argtypes = [POINTER(WtSplitDesc), c_void_p]
    lib.wt_encode_rvq.argtypes = [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]
    lib.wt_encode_rvq_mixed.argtypes = [c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]
    lib.wt_quantize.argtypes = [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]
    lib.wt_vq_residual_probe.argtypes = [POINTER(WtVqResidualDesc), POINTER(WtVqResidualForm), c_void_p]
    lib.wt_model_codebook_tables.argtypes = [c_void_p, c_int32, POINTER(c_void_p), POINTER(c_void_p), POINTER(c_float)]
    lib.wt_mel_create.argtypes = [c_int32, c_int32, c_int32, c_int32, c_int32, POINTER(c_void_p)]
    lib.wt_mel_destroy.argtypes = [c_void_p]
    lib.wt_mel_destroy.restype = None
    lib.wt_mel_frames.argtypes = [c_void_p, c_int64]
    lib.wt_mel_frames.restype = c_int64
    lib.wt_mel_tables.argtypes = [c_int32, c_int32, c_int32, c_void_p, c_void_p]
    lib.wt_mel_workspace_bytes.argtypes = [c_int32, c_int64]
    lib.wt_mel_workspace_bytes.restype = c_size_t
    lib.wt_mel_spectrogram.argtypes = [c_void_p, POINTER(WtMelClip), c_int32, c_int32, c_void_p, c_void_p]
    lib.wt_mel_distance.argtypes = [c_void_p, POINTER(WtMelClip), c_int32, c_void_p, c_void_p]
    lib.wt_stoi_create.argtypes = [c_int32, c_int32, POINTER(c_void_p)]
    lib.wt_stoi_destroy.argtypes = [c_void_p]
    lib.wt_stoi_destroy.restype = None
    lib.wt_stoi_resampled_length.argtypes = [c_void_p, c_int64]
    lib.wt_stoi_resampled_length.restype = c_int64
    lib.wt_stoi_tables.argtypes = [c_int32, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32), c_void_p, c_void_p, c_void_p]
    lib.wt_stoi_workspace_bytes.argtypes = [c_void_p, c_int32, c_int64, c_int64]
    lib.wt_stoi_workspace_bytes.restype = c_size_t
    lib.wt_stoi.argtypes = [c_void_p, POINTER(WtStoiClip), c_int32, c_int32, c_void_p, c_void_p, POINTER(WtStoiTaps)]
    lib.wt_stftd_create.argtypes = [c_int32, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32), c_int32, POINTER(c_void_p)]
    lib.wt_stftd_destroy.argtypes = [c_void_p]
    lib.wt_stftd_destroy.restype = None
    lib.wt_stftd_frames.argtypes = [c_void_p, c_int32, c_int64]
    lib.wt_stftd_frames.restype = c_int64
    lib.wt_stftd_tables.argtypes = [c_int32, c_int32, c_void_p]
    lib.wt_stftd_workspace_bytes.argtypes = [c_void_p, c_int32, c_int64]
    lib.wt_stftd_workspace_bytes.restype = c_size_t
    lib.wt_stftd_distance.argtypes = [c_void_p, POINTER(WtStftdClip), c_int32, c_void_p, c_void_p]
    lib.wt_stftd_magnitude.argtypes = [c_void_p, c_int32, POINTER(WtStftdClip), c_int32, c_void_p, c_void_p]
    lib.wt_wavedist_workspace_bytes.argtypes = [c_int32, c_int64]
    lib.wt_wavedist_workspace_bytes.restype = c_size_t
    lib.wt_wavedist_block.argtypes = []
    lib.wt_wavedist.argtypes = [POINTER(WtWavedistClip), c_int32, c_int32, c_void_p, c_void_p]
    lib.wt_pitch_create.argtypes = [c_int32, POINTER(c_void_p)]
    lib.wt_pitch_destroy.argtypes = [c_void_p]
    lib.wt_pitch_destroy.restype = None
    lib.wt_pitch_frames.argtypes = [c_int64]
    lib.wt_pitch_frames.restype = c_int64
    lib.wt_pitch_tables.argtypes = [c_void_p, c_void_p]
    lib.wt_pitch_workspace_bytes.argtypes = [c_int32, c_int64]
    lib.wt_pitch_workspace_bytes.restype = c_size_t
    lib.wt_pitch_track.argtypes = [c_void_p, POINTER(WtPitchClip), c_int32, c_float, c_float, c_float, c_void_p, c_void_p]
    lib.wt_pitch_pairs.argtypes = [c_void_p, POINTER(WtPitchPair), c_int32, c_float, c_float, c_float, c_void_p, c_void_p]
    lib.wt_level_chunk.argtypes = []
    lib.wt_level_chunk.restype = c_int32
    lib.wt_level_workspace_bytes.argtypes = [c_int32, c_int64]
    lib.wt_level_workspace_bytes.restype = c_size_t
    lib.wt_level.argtypes = [POINTER(WtLevelClip), c_int32, c_void_p, c_void_p]
    lib.wt_normalize_rows_workspace_bytes.argtypes = [c_int32, c_int64]
    lib.wt_normalize_rows_workspace_bytes.restype = c_size_t
    lib.wt_normalize_rows.argtypes = [c_void_p, c_int32, c_int64, POINTER(c_int64), c_int32, c_float, c_void_p, c_void_p, c_void_p]
    lib.wt_scale_rows.argtypes = [c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_void_p]
    lib.wt_emit_rescaled_workspace_bytes.argtypes = [c_int32]
    lib.wt_emit_rescaled_workspace_bytes.restype = c_size_t
    lib.wt_emit_rescaled.argtypes = [POINTER(WtEmitClip), c_int32, c_void_p, c_void_p]
    lib.wt_loudness_chunk.argtypes = []
    lib.wt_loudness_chunk.restype = c_int32
    lib.wt_loudness_blocks.argtypes = [c_int64, c_int32]
    lib.wt_loudness_blocks.restype = c_int64
    lib.wt_kweight_coefficients.argtypes = [c_int32, POINTER(ctypes.c_double)]
    lib.wt_loudness_workspace_bytes.argtypes = [c_int32, c_int64]
    lib.wt_loudness_workspace_bytes.restype = c_size_t
    lib.wt_loudness.argtypes = [POINTER(WtLoudnessClip), c_int32, c_int32, c_void_p, c_void_p]
    lib.wt_normalize_rows_lufs_workspace_bytes.argtypes = [c_int32, c_int64]
    lib.wt_normalize_rows_lufs_workspace_bytes.restype = c_size_t
    lib.wt_normalize_rows_lufs.argtypes = [c_void_p, c_int32, c_int64, POINTER(c_int64), c_int32, ctypes.c_double, c_void_p, c_void_p,
                                           c_void_p]
    lib.wt_true_peak_tile.argtypes = []
    lib.wt_true_peak_tile.restype = c_int32
    lib.wt_true_peak_workspace_bytes.argtypes = [c_int32, c_int64]
    lib.wt_true_peak_workspace_bytes.restype = c_size_t
    lib.wt_true_peak.argtypes = [POINTER(WtTruePeakClip), c_int32, c_int32, c_void_p, c_void_p]
    lib.wt_short_term_blocks.argtypes = [c_int64, c_int32]
    lib.wt_short_term_blocks.restype = c_int64
    lib.wt_loudness_range_workspace_bytes.argtypes = [c_int32, c_int64]
    lib.wt_loudness_range_workspace_bytes.restype = c_size_t
    lib.wt_loudness_range.argtypes = [POINTER(WtLoudnessRangeClip), c_int32, c_int32, c_void_p, c_void_p]
    lib.wt_normalize_rows_lufs_tp_workspace_bytes.argtypes = [c_int32, c_int64]
    lib.wt_normalize_rows_lufs_tp_workspace_bytes.restype = c_size_t
    lib.wt_normalize_rows_lufs_tp.argtypes = [c_void_p, c_int32, c_int64, POINTER(c_int64), c_int32, ctypes.c_double, ctypes.c_double,
                                              c_void_p, c_void_p, c_void_p]
    return lib


lib = _load()


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib.wt_last_error()
        raise WavTokError(f"{what} failed (status {rc}): {msg.decode() if msg else ''}", rc)


# Tensors and streams across the C ABI, for audio.py, engine.py and metrics.py (which import torch; nothing here needs it to load)
def _ptr(t) -> c_void_p:
    """A tensor's data pointer; None gives a null pointer."""
    return c_void_p(t.data_ptr() if t is not None else 0)


def _stream(device) -> c_void_p:
    """The HIP stream that is current on the device."""
    import torch
    return c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _need_gpu(t, message: str) -> None:
    """RuntimeError(message), the calling module's own wording, for a tensor that is not on the GPU."""
    if t.device.type != "cuda":
        raise RuntimeError(message)
