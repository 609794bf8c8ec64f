"""wavtokenizer_amd — MI355X-native WavTokenizer encode/decode path.

``from wavtokenizer_amd import WavTokenizer`` is a drop-in for the reference's
``from decoder.pretrained import WavTokenizer`` (decoder/pretrained.py:32).
Importing the class loads the HIP C-ABI library; it raises if the library is missing.
Beyond the reference's surface the class batches clips of different lengths (``encode_infer_many``, ``decode_many``) and
goes straight between PCM and codes: ``encode_codes`` / ``encode_codes_many`` in, ``decode_codes`` / ``decode_codes_many`` and
``decode_pcm`` / ``decode_pcm_many`` (any rate, mono or stereo, fp32 or int16, one flat tensor) out; recordings longer than a
plan takes go through in overlapping segments (``encode_codes_segmented`` / ``decode_pcm_segmented``, ``wavtokenizer_amd.segmented``).
How good the audio is that comes back: ``wavtokenizer_amd.metrics`` (log-mel L1 distance, the reference's val/mel_loss; STOI and
ESTOI, the intelligibility measure of its evaluation script; the multi-resolution STFT distance, SI-SDR and SNR),
``WavTokenizer.round_trip_mel_distance``, ``WavTokenizer.round_trip_stoi`` and, for all of them from one pass through the codec,
``WavTokenizer.round_trip_report``.
"""
from .config import ArchConfig, ARCH_HOP600, ARCH_HOP320, NAMED_ARCHS, arch_from_yaml  # noqa: F401

__all__ = ["WavTokenizer", "ArchConfig", "ARCH_HOP600", "ARCH_HOP320", "NAMED_ARCHS", "arch_from_yaml"]


def __getattr__(name):
    if name == "WavTokenizer":
        from .pretrained import WavTokenizer
        return WavTokenizer
    raise AttributeError(name)
