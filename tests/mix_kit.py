"""What the PCM mix tests share (tests/test_pcm_mix_*.py): the rule of include/aacgpu.h (aacg_pipeline_set_mix) in numpy float32, the
matrices they mix with, and the standard downmix's table in numpy float64."""
import numpy as np

# the positions the resident route deals out, by channel count (include/aacgpu.h, aacg_mix_standard)
POSITIONS = {1: ["C"], 2: ["L", "R"], 3: ["C", "L", "R"], 4: ["C", "L", "R", "Cs"], 5: ["C", "L", "R", "Ls", "Rs"],
             6: ["C", "L", "R", "Ls", "Rs", "LFE"], 8: ["C", "Lc", "Rc", "L", "R", "Ls", "Rs", "LFE"]}


def mix_rule(pcm, matrix):
    """The rule: pcm (..., C) float32 or int16, matrix (O, C) -> (..., O) of pcm's dtype.  acc = M[o][0] * x[0], then acc = acc +
    M[o][c] * x[c] for c = 1 .. C-1: every product and every sum a float32 operation of its own.  int16: the samples converted to
    float, the sum rounded to nearest even and saturated."""
    pcm = np.asarray(pcm)
    m = np.ascontiguousarray(matrix, np.float32)
    assert m.ndim == 2 and m.shape[1] == pcm.shape[-1] and pcm.dtype in (np.float32, np.int16)
    x = pcm.astype(np.float32)
    rows = []
    for o in range(m.shape[0]):
        acc = m[o, 0] * x[..., 0]
        for c in range(1, m.shape[1]):
            acc = acc + m[o, c] * x[..., c]
        assert acc.dtype == np.float32
        rows.append(acc)
    acc = np.stack(rows, axis=-1)
    if pcm.dtype == np.int16:
        return np.clip(np.rint(acc), -32768, 32767).astype(np.int16)
    return acc


def hostile_matrix(out_channels, channels):
    """distinct coefficients, none a dyadic fraction, signs alternating, every other one above 1"""
    mag = np.array([1.3, 0.67, 1.04, 0.41, 1.78, 0.15, 2.15, 0.52])
    m = np.array([[(-1.0) ** (c + o) * (mag[c] + 0.13 * o) for c in range(channels)] for o in range(out_channels)])
    return m.astype(np.float32)


def standard_table(channels, out_channels, surround_gain, normalise):
    """aacg_mix_standard's table in float64, each coefficient rounded to float32 once.  surround_gain: the float32 the call receives."""
    a, h = float(np.float32(surround_gain)), 1.0 / np.sqrt(2.0)
    left = {"L": 1.0, "Lc": 1.0, "C": h, "Ls": a, "Cs": a * h}
    right = {"R": 1.0, "Rc": 1.0, "C": h, "Rs": a, "Cs": a * h}
    rows = []
    for gains in (left, right):
        row = [float(gains.get(p, 0.0)) for p in POSITIONS[channels]]
        if normalise:
            total = 0.0
            for g in row:
                total += g
            row = [g / total for g in row]
        rows.append(row)
    if out_channels == 1:
        rows = [[(l + r) * 0.5 for l, r in zip(*rows)]]
    return np.array(rows, np.float64).astype(np.float32)
