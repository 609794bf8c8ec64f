"""CPU reference and checks for residual VQ encode (tests/test_rvq_host.py on the CPU, tests/test_rvq.py and
tests/test_rvq_ops.py on the GPU): ResidualVectorQuantizer.encode (encoder/quantization/vq.py:159-168) ->
LanguageVectorQuantization.encode (core_vq.py:403-413), greedy: the nearest row of codebook k to the residual (core_vq.py:175-183,
lowest index on ties), subtract it, go to codebook k + 1.

Two properties carry the checks.  The subtraction is one fp32 rounding per element, so given the codes of the rounds < k the
residual r_k is reproduced here bit for bit, whatever chose those codes: the teacher-forced checker rebuilds r_k from the codes
under test and asks tests/vq_ref.check_codes whether code k is an answer fp32 allows for (r_k, E_k).  And the search is greedy:
the codes of n_q = K are the first K rows of n_q = K + 1.  Built from the definition, never from a kernel output.  CPU only."""
import copy

import torch

from tests import vq_ref as V

MAX_UNDECIDABLE = 0.05       # at most this share of a test's frames may be left out as undecidable: a condition, not a measurement


def rows_of(x):
    """(B, D, L) features -> [B * L][D] rows, as VectorQuantization.encode flattens them (b d n -> b n d -> (b n) d)."""
    return x.float().transpose(1, 2).reshape(-1, x.shape[1])


def nearest(r, e):
    """EuclideanCodebook.quantize (core_vq.py:175-183) in torch fp32, the reference's own expression."""
    embed = e.t()
    dist = -(r.pow(2).sum(1, keepdim=True) - 2 * r @ embed + embed.pow(2).sum(0, keepdim=True))
    return dist.max(dim=-1).indices


def encode(x, codebooks, n_q):
    """x (B, D, L), codebooks [K][bins][D] -> codes (n_q, B, L) int64: the rounds of core_vq.py:403-413 in torch fp32."""
    B, _D, L = x.shape
    r = rows_of(x)
    out = []
    for k in range(n_q):
        c = nearest(r, codebooks[k])
        out.append(c)
        r = r - codebooks[k][c]
    return torch.stack(out).reshape(n_q, B, L)


def residuals(x_rows, codebooks, codes):
    """[r_0 .. r_{K-1}] for the given codes [K][rows]: r_0 = x, r_{k+1} = fl(r_k - E_k[code_k]), the bits a correct kernel holds."""
    r = x_rows.float()
    out = []
    for k in range(codes.shape[0]):
        out.append(r)
        r = r - codebooks[k][codes[k].long().clamp(0, codebooks[k].shape[0] - 1)]
    return out


def num_quantizers_for_bandwidth(bins, n_layers, frame_rate, bandwidth):
    """K of quantizer.encode: vq.py:142-151, cut to the number of layers (core_vq.py:407)."""
    import math
    n_q = n_layers
    if bandwidth and bandwidth > 0.:
        n_q = int(max(1, math.floor(bandwidth * 1000 / (math.log2(bins) * frame_rate))))
    return min(n_q, n_layers)


def _row(ref, m):
    """The one-row view of a tests/vq_ref.Ref (its distances, bounds and duplicate groups are per row already)."""
    one = copy.copy(ref)
    one.rows = 1
    one.nan_rows, one.ovf_rows, one.plain = ref.nan_rows[m:m + 1], ref.ovf_rows[m:m + 1], ref.plain[m:m + 1]
    one.d, one.b = ref.d[m:m + 1], ref.b[m:m + 1]
    return one


def undecidable_rows(x_rows, codebooks, codes, kernel, ees=None):
    """[K][rows] bool: frame m is undecidable in round k when tests/vq_ref.undecidable says so for (r_k[m], E_k) with the kernel's
    bound and the model's own |e|^2 table, r_k rebuilt from the given codes."""
    out = []
    for k, r in enumerate(residuals(x_rows, codebooks, codes)):
        ref = V.Ref(r, codebooks[k], kernel, None if ees is None else ees[k])
        out.append(torch.tensor([V.undecidable(_row(ref, m))[0] > 0 for m in range(ref.rows)]))
    return torch.stack(out)


def check_teacher_forced(codes, x_rows, codebooks, kernel, ees=None, what="rvq"):
    """codes [K][rows] under test: per round k, r_k is rebuilt from the rows < k and tests/vq_ref.check_codes decides whether
    code k is one fp32 allows (exactly the lowest maximising index where the row is decidable).  Returns per round
    (decidable rows, ordinary rows)."""
    codes = torch.as_tensor(codes).reshape(codes.shape[0], -1).long()
    out = []
    for k, r in enumerate(residuals(x_rows, codebooks, codes)):
        out.append(V.check_codes(codes[k], r, codebooks[k], kernel, None if ees is None else ees[k], what=f"{what}: round {k}"))
    return out


def check_against(codes, want, x_rows, codebooks, kernel, ees=None, what="rvq", cap=MAX_UNDECIDABLE):
    """codes against the reference's `want` (both [K][rows]): a frame may differ in round k only if it is undecidable in a round
    <= k (on the reference's own residuals: up to the first difference they are the frame's too), and at most `cap` of the frames
    may be left out this way.  Returns the number of frames left out."""
    codes = torch.as_tensor(codes).reshape(want.shape[0], -1).long()
    want = torch.as_tensor(want).reshape(want.shape[0], -1).long()
    und = undecidable_rows(x_rows, codebooks, want, kernel, ees)
    out_of = torch.cumsum(und.long(), 0) > 0             # round k and the later rounds of an undecidable frame
    left_out = int(out_of[-1].sum())
    assert left_out <= cap * want.shape[1], f"{what}: {left_out} of {want.shape[1]} frames undecidable, more than {cap:.0%}"
    bad = (codes != want) & ~out_of
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} decidable codes differ from the fixture, e.g. (round, frame) {bad.nonzero()[:4].tolist()}"
    return left_out
