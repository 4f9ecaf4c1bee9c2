"""Cases of tests/test_maxsim_ks_gpu.py: the embedding widths between the ones the other MaxSim suites use.  Those suites
run E in {32, 64, 128, 256}, so of the eight instantiations KS = E / 32 that every kernel of the family has
(polus_amd/csrc/maxsim_common.h MS_BY_KS), KS = 3, 5, 6 and 7 are reached by the cases here alone."""

ES = (96, 160, 192, 224)
MODES = ("f32", "bf16")
LQS = (5, 100)                         # one query tile: the query stays in registers; seven: rounds over the document
Q, N, LD = 3, 9, 37                    # Ld = 37: three document tiles, an odd count, the last one partial
C = 7                                  # rerank_cases.candidates plants its absent ids from C = 7 on
TUPLE_N = 3                            # Q * TUPLE_N = N: the corpus is also the tuple buffer, in either layout
NBITS, K = 2, 16                       # the residual codec


def shape(E, Lq):
    """(Q, N, Lq, Ld, E), the form of tests/rerank_cases.SHAPES."""
    return (Q, N, Lq, LD, E)


def tiles_per_wave(E, mode):
    """MsTiles<T, KS>::UT of maxsim_common.h, restated: (64 / FR) / KS clamped to 1..8, FR = 4 (bf16) or 8 (f32)."""
    fr = 4 if mode == "bf16" else 8
    return max(1, min(8, (64 // fr) // (E // 32)))


def route(E, mode, Lq):
    """"registers" where the query's 16-token tiles fit one wave (the RES = true kernels), else "rounds"."""
    return "registers" if -(-Lq // 16) <= tiles_per_wave(E, mode) else "rounds"
