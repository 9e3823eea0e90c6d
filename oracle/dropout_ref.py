"""numpy restatement of the decoders' dropout mask. TEST INFRASTRUCTURE.

The library draws its mask from a counter hash (csrc/dropout_mask.h, dropout_scale(seed, sample, col, e, p, inv_keep)),
computed again wherever it is needed instead of being stored. This file states that hash a second time in uint64
arithmetic (which wraps, as the C does), so the CPU oracle can run with the very masks the kernels drew:

  z = seed + 0x9E3779B97F4A7C15 * ((((sample << 20) ^ (col << 10)) * 1000003) + e + 1)
  z = splitmix64 finaliser of z
  u = float32(z >> 40) * 2^-24                 (exact: 24 bits)
  keep iff u >= float32(p); a kept unit is scaled by float32(1) / (float32(1) - float32(p)), correctly rounded.

Coordinates, as the kernels pass them:
  * the input embeddings (gather_inputs / scatter_input_grad, seq_kernels.hip, rows laid out by build_rows):
    sample = batch index, col = CAPTION COLUMN the row reads, e = unit. Only teacher-forced rows are masked; the
    image-feature row and every free-running row (B(predicted), and B(captions[:, 0]) of a free-running first step)
    are not. With image features step t reads column t - 1, without them column t; either way the mask entry is the
    one of the column read, so one [B, T, E] array indexed by caption column serves both -- the layout
    oracle.decoders_ref's drop_mask multiplies into B(captions) before the feature row is prepended.
  * between stacked layers (rows_dropout, seq_kernels.hip; the fused step lstm_upper_step.hip): the input of layer
    l > 0 at packed row r (time-major, pack_padded_sequence order: the rows of step t are off[t] .. off[t] + bs[t] - 1)
    is h^{l-1}[r] * dropout_scale(seed, r, 0x40000000 + l, e). The column slot carries the layer, offset out of the
    caption columns' range.
"""
import numpy as np

_U64 = np.uint64
LAYER_COL_BASE = 0x40000000


def keep_scale(p):
    """float32(1) / (float32(1) - float32(p)): the value of a kept unit."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def dropout_scale(seed, sample, col, e, p):
    """Elementwise dropout_scale over broadcastable integer arrays -> float32 array of 0 or keep_scale(p)."""
    sample = np.asarray(sample, dtype=np.int64).astype(_U64)
    col = np.asarray(col, dtype=np.int64).astype(_U64)
    e = np.asarray(e, dtype=np.int64).astype(_U64)
    with np.errstate(over="ignore"):
        k = ((sample << _U64(20)) ^ (col << _U64(10))) * _U64(1000003) + e + _U64(1)
        z = _U64(seed) + _U64(0x9E3779B97F4A7C15) * k
        z = (z ^ (z >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U64(27))) * _U64(0x94D049BB133111EB)
        z = z ^ (z >> _U64(31))
    u = (z >> _U64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return np.where(u >= np.float32(p), keep_scale(p), np.float32(0.0)).astype(np.float32)


def embedding_mask(seed, B, T, E, p):
    """[B, T, E] float32 mask of the input embeddings: sample = batch index, col = caption column, e = unit."""
    return dropout_scale(seed, np.arange(B).reshape(B, 1, 1), np.arange(T).reshape(1, T, 1),
                         np.arange(E).reshape(1, 1, E), p)


def layer_mask(seed, N, H, p, layer):
    """[N, H] float32 mask of layer `layer`'s input (layer > 0): sample = packed row, col = 0x40000000 + layer."""
    return dropout_scale(seed, np.arange(N).reshape(N, 1), LAYER_COL_BASE + layer, np.arange(H).reshape(1, H), p)
