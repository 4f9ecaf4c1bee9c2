"""Cases of the entity tests (tests/test_entity_cpu.py, tests/test_entity_gpu.py): tag schemes, the shapes around the
kernels' 64-token step, three kinds of row, and masks.  Everything is generated from a seed; nothing of the package is
imported."""
import numpy as np

BS = (1, 5, 67)                                    # one row; a workgroup of 4 rows and one more; many workgroups
SS = (1, 2, 63, 64, 65, 129, 300)                  # one-lane rows, both sides of the 64-token step, several steps
KINDS = ("uniform", "wellformed", "edited")
MASKS = ("none", "prefix", "holes", "zero_row", "all_zero")
# (T, C): one type with the reference's four tags; three types; the kernels' limits
SCHEMES = ((1, 4), (3, 8), (128, 256))
MAX_ENTITY = 150                                   # entity lengths reach this: they cross one and two 64-token edges


def scheme_names(T, C):
    """C tag names: PAD, O, then B-t and I-t for every type t, then further outside names up to C.  Where C has no room
    for every I-t (T = 128 with C = 256), the last types have a B-t only."""
    names = ["PAD", "O"]
    for t in range(T):
        names.append(f"B-t{t}")
        if C - len(names) > T - t - 1:             # room left after one B- for each later type
            names.append(f"I-t{t}")
    names += [f"X{k}" for k in range(C - len(names))]
    assert len(names) == C
    return names


def scheme_table(T, C):
    """int32 [C] by hand from the names: -1 outside, 2 * type + (1 for I-)."""
    out = []
    for n in scheme_names(T, C):
        out.append(2 * int(n[3:]) + (n[0] == "I") if n[:3] in ("B-t", "I-t") else -1)
    return np.asarray(out, np.int32)


def _rng(*key):
    return np.random.Generator(np.random.PCG64([int(k) for k in key]))


def _tag(scheme, code):
    """The first tag id with this code, None if the scheme has none."""
    at = np.nonzero(scheme == code)[0]
    return int(at[0]) if at.size else None


def uniform_rows(B, S, scheme, seed=0):
    """Uniform random tags: heavily malformed, with many I after O and type changes."""
    return _rng(11, B, S, len(scheme), seed).integers(0, len(scheme), size=(B, S)).astype(np.int32)


def wellformed_rows(B, S, scheme, seed=0):
    """Rows of O with random entities B-t I-t ... whose lengths reach MAX_ENTITY, some of them adjacent."""
    r = _rng(12, B, S, len(scheme), seed)
    T = int(scheme.max()) // 2 + 1
    o = _tag(scheme, -1)
    out = np.full((B, S), o, np.int32)
    for b in range(B):
        col = int(r.integers(0, 3))
        while col < S:
            t = int(r.integers(0, T))
            n = int(r.integers(1, MAX_ENTITY + 1)) if r.random() < 0.3 else int(r.integers(1, 6))
            inside = _tag(scheme, 2 * t + 1)
            n = min(n, S - col) if inside is not None else 1
            out[b, col] = _tag(scheme, 2 * t)
            if n > 1:
                out[b, col + 1:col + n] = inside
            col += n + int(r.integers(0, 4))
    return out


def edited_rows(gold, scheme, seed=0):
    """A copy of gold with random single-tag edits (about one token in twelve), row 0 left equal to gold."""
    r = _rng(13, gold.shape[0], gold.shape[1], len(scheme), seed)
    out = gold.copy()
    hit = r.random(gold.shape) < 1.0 / 12
    hit[0] = False
    out[hit] = r.integers(0, len(scheme), size=int(hit.sum())).astype(np.int32)
    return out


def make_pair(kind, B, S, scheme, seed=0):
    """(a, b) int32 [B, S]: the gold side and the predicted side of one case."""
    if kind == "uniform":
        return uniform_rows(B, S, scheme, seed), uniform_rows(B, S, scheme, seed + 1000)
    gold = wellformed_rows(B, S, scheme, seed)
    if kind == "wellformed":
        return gold, wellformed_rows(B, S, scheme, seed + 1000)
    assert kind == "edited"
    return gold, edited_rows(gold, scheme, seed)


def make_mask(which, B, S, seed=0):
    """int32 [B, S] or None.  prefix: lengths in [0, S] with 1 and S among them; holes: about a third of the tokens
    dropped, runs longer than a 64-token step among them; zero_row: holes with the middle row empty; all_zero."""
    if which == "none":
        return None
    r = _rng(14, B, S, MASKS.index(which), seed)
    if which == "all_zero":
        return np.zeros((B, S), np.int32)
    if which == "prefix":
        n = r.integers(0, S + 1, size=B)
        n[0] = S
        n[-1] = 1
        return (np.arange(S)[None] < n[:, None]).astype(np.int32)
    m = (r.random((B, S)) >= 0.3).astype(np.int32) * r.integers(1, 4, size=(B, S)).astype(np.int32)   # any nonzero keeps
    if S > 80:
        for b in range(0, B, 2):                   # a hole longer than one step, over a step edge
            s0 = int(r.integers(0, S - 80))
            m[b, s0:s0 + 70] = 0
    if which == "zero_row":
        m[B // 2] = 0
    return m


def planted(S, scheme):
    """Rows [5, S] of O with one planted entity each, as far as S has the room: it starts at 63, ends at 63 (last token
    63), ends at 64, spans 0..S-1, and a B-t at the very last token.  Returns (tags, the entities per row)."""
    o, b_, i_ = _tag(scheme, -1), _tag(scheme, 0), _tag(scheme, 1)
    tags = np.full((5, S), o, np.int32)
    want = [[] for _ in range(5)]

    def put(row, s, e):
        if 0 <= s < e <= S:
            tags[row, s] = b_
            tags[row, s + 1:e] = i_
            want[row].append((s, e, 0))
    put(0, 63, min(S, 70))
    put(1, 60, 64)
    put(2, 60, 65)
    put(3, 0, S)
    put(4, S - 1, S)
    return tags, want
