"""The yardstick of tests/test_i8_slices_cpu.py and tests/test_gpu_i8_slices.py: the contract at the head of csrc/kernels_i8.hip for cutting
an fp64 operand V[rows_pad][b] into S int8 digit planes, restated in int64 / Python-int arithmetic.  Nothing here calls the library.

  x       = v * rowscale[row] (one fp64 product; no rowscale: v itself), rows >= rows count as zero
  e_c     : 2^e_c > max_r |x[r][c]| from frexp of the column maximum (0.5 <= f < 1); a zero column has e_c = 0.  Another rank may hold a
            larger maximum: the exponent comes from the largest one installed
  F       = 8 S - 2;  m = rint(x 2^(F - e_c)), ties to even, |m| <= 2^F
  digits  : m = sum_i d_i 256^i, d_i in [-128, 127] for i < S - 1 (the low byte read as signed, the rest carried), d_{S-1} what remains
            (within +-64 by |m| <= 2^F); slice s holds digit S - 1 - s: slice 0 is the top one
  Q       : [S b][rows_pad], Q[s b + c][16 g + 4 q + t] = digit of row 16 g + q + 4 t;  Qrm: [rows_pad][S b], Qrm[row][s b + c]
  colw    : [nsc_pad], colw[s b + c] = 2^(e_c - F + 8 (S - 1 - s)), exact zeros from S b on
  colsum  : [S b], the integer sum of every plane's digits
  copies  : k_slice leaves x itself (fp64) or float32(x 2^(1 - e_c)); the exchange kernels m 2^(e_c - F) or float32(m 2^(1 - F)), rows <
            rows_valid; what is not written keeps the poison
"""
import numpy as np

GROUP_ROW = np.array([p // 4 + 4 * (p % 4) for p in range(16)])  # position p of a 16-row group holds row GROUP_ROW[p]
POISON_BYTE = 0x55
SHARDS, CS_STRIDE = 8, 640


def scaled(V, rows, rowscale=None):
    """x [rows_pad][b]: v * rowscale for rows < rows, zero behind."""
    V = np.asarray(V, dtype=np.float64)
    x = np.zeros_like(V)
    x[:rows] = V[:rows] if rowscale is None else V[:rows] * np.asarray(rowscale, dtype=np.float64)[:rows, None]
    return x


def column_maxima(x):
    return np.abs(x).max(axis=0) if x.shape[0] else np.zeros(x.shape[1])


def exponents(colmax):
    """e_c of every column; zero column -> 0."""
    f, e = np.frexp(np.asarray(colmax, dtype=np.float64))
    assert np.all((f == 0) | ((f >= 0.5) & (f < 1)))
    return np.where(f == 0, 0, e).astype(np.int64)


def fixed_point(x, e, S):
    """m [rows_pad][b] int64 = rint(x 2^(F - e_c)), ties to even."""
    F = 8 * S - 2
    y = np.ldexp(x, (F - e)[None, :].astype(np.int32))  # exact: a power of two (results below 2^-1022 are far below 1/2 either way)
    m = np.rint(y)
    assert np.all(np.abs(m) <= 2.0 ** F)
    return m.astype(np.int64)


def digits(m, S):
    """D [S][rows_pad][b] int8 by slice: D[0] the top digit.  The top digit is what remains and is asserted to fit, not wrapped."""
    D = np.empty((S,) + m.shape, dtype=np.int8)
    rest = m.copy()
    for i in range(S - 1):
        d = ((rest + 128) & 255) - 128  # the low byte as a signed number
        D[S - 1 - i] = d
        rest = (rest - d) >> 8          # exact: rest - d is a multiple of 256
    assert np.all(np.abs(rest) <= 64), "top digit outside +-64"
    D[0] = rest
    return D


def q_layout(D):
    """Q [S b][rows_pad] from D [S][rows_pad][b]."""
    S, rows_pad, b = D.shape
    planes = D.transpose(0, 2, 1).reshape(S * b, rows_pad // 16, 16)
    return np.ascontiguousarray(planes[:, :, GROUP_ROW]).reshape(S * b, rows_pad)


def qrm_layout(D):
    """Qrm [rows_pad][S b]."""
    S, rows_pad, b = D.shape
    return np.ascontiguousarray(D.transpose(1, 0, 2)).reshape(rows_pad, S * b)


def weights(e, S, nsc_pad):
    b = e.size
    w = np.zeros(nsc_pad)
    for s in range(S):
        w[s * b:(s + 1) * b] = np.ldexp(1.0, (e - (8 * S - 2) + 8 * (S - 1 - s)).astype(np.int32))
    return w


def column_sums(D):
    S, rows_pad, b = D.shape
    return D.sum(axis=1, dtype=np.int64).reshape(S * b)


class Sliced:
    """Everything the contract fixes for one operand.  colmax: the maxima the exponents come from (default: the operand's own)."""

    def __init__(self, V, rows, S, nsc_pad, rowscale=None, colmax=None):
        self.S, self.rows, (self.rows_pad, self.b) = S, rows, np.shape(V)
        self.F = 8 * S - 2
        self.x = scaled(V, rows, rowscale)
        self.own_max = column_maxima(self.x)
        self.colmax = self.own_max if colmax is None else np.asarray(colmax, dtype=np.float64)
        assert np.all(self.colmax >= self.own_max)
        self.e = exponents(self.colmax)
        self.m = fixed_point(self.x, self.e, S)
        self.D = digits(self.m, S)
        self.nsc_pad = nsc_pad
        self.colw = weights(self.e, S, nsc_pad)
        self.colsum = column_sums(self.D)

    def Q(self):
        """[nsc_pad][rows_pad]: the slices, and the poison the kernels must leave in the padding slice-columns."""
        q = np.full((self.nsc_pad, self.rows_pad), POISON_BYTE, dtype=np.int8)
        q[:self.S * self.b] = q_layout(self.D)
        return q

    def Qrm(self):
        return qrm_layout(self.D)

    # the copies as bit patterns' owners: NaN = poison (compare as unsigned views)
    def slice_copy64(self):
        out = _poison(self.x.shape, np.float64)
        out[:self.rows] = self.x[:self.rows]
        return out

    def slice_copy32(self):
        out = _poison(self.x.shape, np.float32)
        out[:self.rows] = np.ldexp(self.x[:self.rows], (1 - self.e)[None, :].astype(np.int32)).astype(np.float32)
        return out

    def exchange_copy64(self, rows_valid):
        out = _poison(self.x.shape, np.float64)
        out[:rows_valid] = np.ldexp(self.m[:rows_valid].astype(np.float64), (self.e - self.F)[None, :].astype(np.int32))
        return out

    def exchange_copy32(self, rows_valid):
        assert self.S <= 4  # |m| <= 2^30: exact in fp64, one rounding to fp32
        out = _poison(self.x.shape, np.float32)
        out[:rows_valid] = np.ldexp(self.m[:rows_valid].astype(np.float64), 1 - self.F).astype(np.float32)
        return out


def _poison(shape, dtype):
    """All bits set, as the hook fills the copies."""
    return np.full(shape, -1, dtype=np.int32 if dtype == np.float32 else np.int64).view(dtype)


def bits(a):
    """A float array as its bit patterns (NaN payloads included): what the exact comparisons compare."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def fold_maxbits(raw):
    """[8][64] uint64 bit patterns of non-negative doubles -> the 64 maxima (they order like integers)."""
    return np.asarray(raw, dtype=np.uint64).reshape(SHARDS, 64).max(axis=0).view(np.float64)


def python_int_value(D, row, col):
    """sum_i d_i 256^i of one entry in Python ints (slice 0 = top)."""
    S = D.shape[0]
    return sum(int(D[s, row, col]) * 256 ** (S - 1 - s) for s in range(S))
