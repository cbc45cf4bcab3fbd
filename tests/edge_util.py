"""Test helper: carry-edge operands for the field arithmetic of csrc/field.hpp.

Uniform random field elements make the rare branches of the device's 32-bit carry / borrow chains fire about once in
2^32 operations.  The operands here are built from a "limb alphabet" instead: every 32-bit word of an element is 0, 1, 2,
all ones, the sign bit or a neighbour (f64), or a limb of p = 2^128 - C, of C, or a neighbour (f128).
tests/cpp/test_field_edges.cpp measures what these sets are worth: a reduction whose borrow mask drops one term agrees with
the real one on 200 000 000 uniform products and differs on 92 of the 1849 f64 alphabet pairs.

All values are in the library's in-memory form (f64: Montgomery residues, f128: canonical integers); any value below p is a
valid element in either."""
import numpy as np

F64, F128 = 1, 2
P64 = 2**64 - 2**32 + 1
P128 = 2**128 - 45 * 2**40 + 1
R64 = 2**64 % P64            # Montgomery one()
R64_INV = pow(2**64, -1, P64)
MODULUS = {F64: P64, F128: P128}
ONE = {F64: R64, F128: 1}    # the in-memory form of 1

LIMBS64 = (0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF)
LIMBS128 = (0, 1, 0x2CFF, 0x2D00, 0x80000000, 0xFFFFD2FF, 0xFFFFD300, 0xFFFFFFFE, 0xFFFFFFFF)

# edge[] of tests/cpp/test_field_limbs.cpp (the shift twiddles' own list), reduced mod p as there
SHIFT_EDGES = [v % P64 for v in (
    0, 1, 2, 0xFFF, 0x1000, 0xFFFFFF, 0x1000000, 0xFFFFFFFF, 0x100000000, 0xFFFFFFFF00000000, 0xFFFFFFFEFFFFFFFF,
    0xFFFFFFFF00000000 - 1, P64 - 1, P64 - 2, P64 - 0x1000, 0xFFFFF00000000000, 0x000FFFFFFFFFFFFF, 0xFFF0000000000001,
    0x8000000000000000, 0x7FFFFFFFFFFFFFFF, 0x0000FFFFFFFFFFFF, 0x0000FFFF0000FFFF, 0xFFFF0000FFFFFFFF, 0x00000000FFFF0000,
    0x0FFFFFFFFFFFFFFF, 0xFFFFFFFF << 4, 0xFFFFFFFF << 16, 0xFFFFFFFF << 28)]


def f64_alphabet() -> list:
    """The 43 values below p whose two 32-bit halves come from LIMBS64 (6 of the 49 are at or above p)."""
    out = [(hi << 32) | lo for hi in LIMBS64 for lo in LIMBS64 if ((hi << 32) | lo) < P64]
    assert len(out) == 43
    return out


def f128_alphabet() -> list:
    """The 6535 values below p whose four 32-bit limbs come from LIMBS128 (26 of the 6561 are at or above p)."""
    out = []
    for l3 in LIMBS128:
        for l2 in LIMBS128:
            for l1 in LIMBS128:
                for l0 in LIMBS128:
                    v = (l3 << 96) | (l2 << 64) | (l1 << 32) | l0
                    if v < P128:
                        out.append(v)
    assert len(out) == 6535
    return out


def directed_reduction_inputs(n_random: int = 2000, seed: int = 1):
    """(lo, hi) inputs of F64::mont_reduce with hi next to the value b(lo) that the function subtracts from it -- where the
    borrows c1 and c3 and the final d1 fire.  b as the function's comment defines it: a = lo + (lo << 32), b = a - (a >> 32) -
    carry.  hi = b + d for the small and word-sized d below, kept where hi < p (the function's precondition)."""
    M = 2**64
    rng = np.random.default_rng(seed)
    los = f64_alphabet() + [M - 1, P64, P64 + 1, 0x00000001FFFFFFFF, 0x8000000080000000]
    los += rng.integers(0, M - 1, size=n_random, dtype=np.uint64, endpoint=True).tolist()
    ds = [0]
    for d in (1, 2, 2**32 - 1, 2**32, 2**32 + 1):
        ds += [d, -d]
    lo_out, hi_out = [], []
    for lo in los:
        a = (lo + (lo << 32)) % M
        b = (a - (a >> 32) - (1 if a < lo else 0)) % M
        for d in ds:
            hi = (b + d) % M
            if hi < P64:
                lo_out.append(lo)
                hi_out.append(hi)
    return lo_out, hi_out


def u64(values) -> np.ndarray:
    return np.array(values, dtype=np.uint64)


def f128_array(values) -> np.ndarray:
    """Python integers -> (n, 2) uint64 (lo, hi)."""
    vals = list(values)
    out = np.empty((len(vals), 2), dtype=np.uint64)
    out[:, 0] = u64([v & 0xFFFFFFFFFFFFFFFF for v in vals])
    out[:, 1] = u64([v >> 64 for v in vals])
    return out


def f128_ints(arr) -> list:
    a = np.asarray(arr, dtype=np.uint64).reshape(-1, 2)
    return [lo | (hi << 64) for lo, hi in a.tolist()]


def elements(field: int, values) -> np.ndarray:
    """Python integers below p -> the array form of `field` ((n,) uint64 or (n, 2) uint64)."""
    return u64(values) if field == F64 else f128_array(values)


_ALPHABET_ARRAYS = {}


def alphabet_array(field: int) -> np.ndarray:
    if field not in _ALPHABET_ARRAYS:
        _ALPHABET_ARRAYS[field] = elements(field, f64_alphabet() if field == F64 else f128_alphabet())
    return _ALPHABET_ARRAYS[field]


def alphabet_draw(rng, field: int, n: int) -> np.ndarray:
    """n elements drawn from the field's limb alphabet."""
    a = alphabet_array(field)
    return a[rng.integers(0, a.shape[0], size=n)].copy()


# "alphabet" and "pm1" come first: a matrix of fewer columns than patterns still gets these two
PATTERNS = ("alphabet", "pm1", "alt", "single_last", "const", "single_0", "zero", "single_1")
_CONST = {F64: 0xFFFFFFFEFFFFFFFF, F128: (0xFFFFFFFFFFFFFFFF << 64) | (0x2D00 << 32)}


def pattern_column(rng, field: int, kind: str, n: int, ext: int = 1) -> np.ndarray:
    """One column of n elements (rows) of `ext` coordinates each, n * ext base-field elements with the coordinates of a row side
    by side: all zero / all p - 1 / one constant / a single non-zero row 0, 1 or n - 1 in zeros / rows alternating between 0 and
    p - 1 / drawn from the limb alphabet.  The patterns are laid over rows, not over base elements: a non-zero row has p - 1
    (or the constant) in every coordinate, a zero row has 0 in every coordinate, and "alphabet" draws every coordinate."""
    p = MODULUS[field]
    if kind == "alphabet":
        return alphabet_draw(rng, field, n * ext)
    if kind == "zero":
        rows = [0] * n
    elif kind == "pm1":
        rows = [p - 1] * n
    elif kind == "const":
        rows = [_CONST[field]] * n
    elif kind == "alt":
        rows = [0, p - 1] * (n // 2) + [0] * (n % 2)
    elif kind.startswith("single_"):
        at = {"single_0": 0, "single_1": min(1, n - 1), "single_last": n - 1}[kind]
        rows = [0] * n
        rows[at] = p - 1
    else:
        raise ValueError(kind)
    return elements(field, [v for v in rows for _ in range(ext)])


def pattern_columns(rng, field: int, n_cols: int, n: int, ext: int = 1, first: int = 0) -> list:
    """n_cols columns of n rows, the patterns of PATTERNS in turn from number `first` on: neighbouring columns of one matrix (the
    lanes of a packed row, the columns of a segment) hold different patterns."""
    return [pattern_column(rng, field, PATTERNS[(first + c) % len(PATTERNS)], n, ext) for c in range(n_cols)]


def single_at(field: int, n: int, ext: int, index: int) -> np.ndarray:
    """One column of n rows of `ext` coordinates: zeros, and p - 1 in every coordinate of row `index`."""
    rows = [0] * n
    rows[index] = MODULUS[field] - 1
    return elements(field, [v for v in rows for _ in range(ext)])


def edge_scalars(field: int) -> list:
    """0, 1 and p - 1 as stored (any value below p is an element; 1 is Montgomery one() for f64), and -1."""
    p = MODULUS[field]
    minus_one = (p - 1) * R64 % p if field == F64 else p - 1
    return sorted({0, ONE[field], p - 1, minus_one, 1})


def edge_points(field: int, ext: int) -> list:
    """Elements of the degree-`ext` extension: (v, 0, ..) for the edge scalars, and for ext > 1 a single non-zero coordinate
    elsewhere (base part 0)."""
    pts = [[v] + [0] * (ext - 1) for v in edge_scalars(field)]
    for k in range(1, ext):
        for v in (ONE[field], MODULUS[field] - 1):
            pt = [0] * ext
            pt[k] = v
            pts.append(pt)
    return [elements(field, pt) for pt in pts]


def edge_points_nonzero(field: int, ext: int) -> list:
    """edge_points without the zero element (the points with base part 0 and another coordinate set stay)."""
    return [pt for pt in edge_points(field, ext) if pt.any()]


def commit_resident_with_polys(ctx, orc, params, polys: list, ext: int):
    """A resident trace commitment whose polynomials are the given coefficient vectors.  trace_commit_resident takes
    evaluations and interpolates them; field arithmetic is exact, so the oracle's evaluations of `polys` over the trace domain
    (no offset) come back as `polys`, which is asserted on the polynomials the call returns.  -> the commitment."""
    field, n = params.field, 1 << params.log2_trace_len
    tw = orc.get_twiddles(field, n)
    cols = []
    for p in polys:
        v = p.copy()
        orc.evaluate_poly(field, v, n, ext, tw)
        cols.append(v)
    com, got = ctx.trace_commit_resident(params, cols, want_polys=True)
    for c, (g, p) in enumerate(zip(got, polys)):
        assert np.array_equal(g, p), f"resident polynomial {c} is not the chosen coefficient vector"
    return com
