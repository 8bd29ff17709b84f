"""Test vectors shared by the CPU layer (test_device_logic.py: the per-lane code on the host harness) and the GPU
layer (test_gpu_device_logic.py, test_gpu_torsion_maxlimb.py: the same code on the device).  Each builder
draws from a seeded generator, so both layers see the same cases."""
import random

import ed25519_ref as E

P, L = E.P, E.L

OFF = [0, 26, 51, 77, 102, 128, 153, 179, 204, 230]
W = [26, 25] * 5


def limb_val(v):
    return sum(int(x) * (1 << o) for x, o in zip(v, OFF))


def limbs(rng, mult):
    """Ten unsigned limbs at, just under, anywhere below, or at zero of mult * 2^w_i (cv_field.h's units)."""
    return [min(int(rng.choice([mult, mult * 0.999, rng.random() * mult, 0.0]) * (1 << W[i])),
                int(mult * (1 << W[i])) - 1) for i in range(10)]


def max_limbs(mult):
    """Every limb at the largest value limbs(rng, mult) can give."""
    return [int(mult * (1 << W[i])) - 1 for i in range(10)]


def field_values(rng):
    """test_field_ops_random_and_extreme's values (below 2^255)."""
    return [0, 1, 2, 19, P - 1, P, P + 1, P + 18, 2**255 - 1, 2**254, 2**128 + 7] + \
           [rng.randrange(2**255) for _ in range(300)]


def sc_reduce_cases(rng):
    cases = [bytes(64), b"\xff" * 64, L.to_bytes(64, "little"), (L - 1).to_bytes(64, "little"),
             (2 * L).to_bytes(64, "little"), (2**512 - L).to_bytes(64, "little")]
    cases += [rng.getrandbits(512).to_bytes(64, "little") for _ in range(3000)]
    return cases


HALFSIZE_EDGES = 7          # the leading cases of halfsize_cases: the only ones allowed to fall back


def halfsize_cases(rng):
    cases = [(0, 0), (1, 5), (L - 1, L - 1), (2**128 - 1, 3), (2**128, 1), (2**252, 7), (8, 9)]
    cases += [(rng.randrange(L), rng.randrange(L)) for _ in range(3000)]
    return cases


def exact_step_cases(rng):
    """(r0, r1) with r0 = k r1 - d, d tiny of either sign or zero, r0 >= r1 >= 2^128."""
    cases = []
    for _ in range(4000):
        r1 = rng.randrange(2 ** 128, 2 ** rng.randrange(129, 225))
        k = rng.choice([1, 2, 3, rng.randrange(2, 2 ** 32), 2 ** 32 - 1, 2 ** rng.randrange(1, 32)])
        for d in (0, 1, 2, rng.randrange(1, 2 ** 20), -1, -rng.randrange(1, 2 ** 20)):
            r0 = k * r1 - d
            if r1 <= r0 < 2 ** 256:
                cases.append((r0, r1))
    return cases


SHA_LENGTHS = [0, 1, 31, 47, 48, 49, 55, 56, 57, 63, 64, 111, 112, 113, 119, 120, 121, 127, 128, 200, 300, 1000]
SHA_SHIFTS = (1, 2, 3, 5)          # unaligned message starts


def tri_digit_scalars(rng):
    """(h, s) of test_tri_digit_words: edge h, nibbles at the recoding's edges, random."""
    hs = [0, 1, 2**128, 2**252, L - 1, 2**253 - 1, int("8" * 63, 16) % L, int("7" * 63, 16) % L]
    hs += [rng.randrange(L) for _ in range(2000)]
    return [(h, rng.randrange(L) if i % 3 else (L - 1 - i)) for i, h in enumerate(hs)]


def max_limb_cases():
    """(encs, cases) of test_limb_bounds_on_max_limb_encodings: the decodable encodings with y in
    [2^255 - 64, 2^255) and y = 2^255 - 2^j, both sign bits, and 184 (pk, sig, msg) over them with S at
    2^256 - 1, 2^255 and around L."""
    rng = random.Random(20261018)
    ys = [(1 << 255) - 1 - k for k in range(64)] + [(1 << 255) - (1 << j) for j in range(1, 255, 7)]
    encs = []
    for y in ys:
        for sign in (0, 1):
            e = (y | (sign << 255)).to_bytes(32, "little")
            try:
                E.decode_point_0_1_0(e)
                encs.append(e)
            except Exception:
                pass
    assert len(encs) >= 40
    svals = [(1 << 256) - 1, 1 << 255, (1 << 255) + 12345, L, L - 1, L + 1, (1 << 253) + rng.getrandbits(200)]
    cases = []
    for _ in range(160):
        pk, r = rng.choice(encs), rng.choice(encs)
        s = rng.choice(svals)
        cases.append((pk, r + s.to_bytes(32, "little"), rng.randbytes(rng.choice([0, 32, 300]))))
    # the same max-limb R over a real key, and honest signatures rewritten to the non-canonical key encoding
    seed = bytes(range(32))
    pk_h = E.public_key_of(seed)
    for r in encs[:24]:
        cases.append((pk_h, r + ((1 << 256) - 1).to_bytes(32, "little"), b"corda"))
    return encs, cases
