"""The fixed-key signing procedures (cv_key_expand, ge_scalarmult_base_w16, cv_sign_keyed_one in
corda_amd/csrc/cv_verify.h) compiled for the CPU (tests/sign_harness.cpp) against the Python oracle.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ed25519_ref as E

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# RFC 8032 section 7.1: (seed, public key, message, signature)
RFC8032 = [
    ("9d61b19deffd5a60ba844af492ec2cc44449c5697b326919703bac031cae7f60",
     "d75a980182b10ab7d54bfed3c964073a0ee172f3daa62325af021a68f707511a", "",
     "e5564300c360ac729086e2cc806e828a84877f1eb8e5d974d873e06522490155"
     "5fb8821590a33bacc61e39701cf9b46bd25bf5f0595bbe24655141438e7a100b"),
    ("4ccd089b28ff96da9db6c346ec114e0f5b8a319f35aba624da8cf6ed4fb8a6fb",
     "3d4017c3e843895a92b70aa74d1b7ebc9c982ccf2ec4968cc0cd55f12af4660c", "72",
     "92a009a9f0d4cab8720e820b5f642540a2b27b5416503f8fb3762223ebdb69da"
     "085ac1e43e15996e458f3613d0f11d8c387b2eaeb4302aeeb00d291612bb0c00"),
    ("c5aa8df43f9f837bedb7442f31dcb7b166d38535076f094b85ce3a2e0b4458f7",
     "fc51cd8e6218a1a38da47ed00230f0580816ed13ba3303ac5deb911548908025", "af82",
     "6291d657deec24024827e69c3abe01a30ce548a284743a445e3680d7db5ac3ac"
     "18ff9b538d16f290ae67f760984dc6594a7c15e9716ed28dc027beceea1ec40a"),
    # TEST SHA(abc): the message is SHA-512("abc")
    ("833fe62409237b9d62ec77587520911e9a759cec1d19755b7da901b96dca3d42",
     "ec172b93ad5e563bf4932c70e1245034c35467ef2efd4d64ebf819683467e2bf",
     "ddaf35a193617abacc417349ae20413112e6fa4e89a97ea20a9eeee64b55d39a"
     "2192992a274fc1a836ba3c23a3feebbd454d4423643ce80e2a9ac94fa54ca49f",
     "dc2a4459e7369633a52b1bf277839a00201009a3efbf3ecb69bea2186c26b589"
     "09351fc9ac90b3ecfdfbc7c66431e0303dca179c138ac17ad9bef1177331a704"),
    # TEST 1024: a 1,023-byte message (eight SHA-512 blocks in both hashes)
    ("f5e5767cf153319517630f226876b86c8160cc583bc013744c6bf255f5cc0ee5",
     "278117fc144c72340f67d0f2316e8386ceffbf2b2428c9c51fef7c597f1d426e",
     "08b8b2b733424243760fe426a4b54908632110a66c2f6591eabd3345e3e4eb98fa6e264bf09efe12ee50f8f54e9f77b1"
     "e355f6c50544e23fb1433ddf73be84d879de7c0046dc4996d9e773f4bc9efe5738829adb26c81b37c93a1b270b20329d"
     "658675fc6ea534e0810a4432826bf58c941efb65d57a338bbd2e26640f89ffbc1a858efcb8550ee3a5e1998bd177e93a"
     "7363c344fe6b199ee5d02e82d522c4feba15452f80288a821a579116ec6dad2b3b310da903401aa62100ab5d1a36553e"
     "06203b33890cc9b832f79ef80560ccb9a39ce767967ed628c6ad573cb116dbefefd75499da96bd68a8a97b928a8bbc10"
     "3b6621fcde2beca1231d206be6cd9ec7aff6f6c94fcd7204ed3455c68c83f4a41da4af2b74ef5c53f1d8ac70bdcb7ed1"
     "85ce81bd84359d44254d95629e9855a94a7c1958d1f8ada5d0532ed8a5aa3fb2d17ba70eb6248e594e1a2297acbbb39d"
     "502f1a8c6eb6f1ce22b3de1a1f40cc24554119a831a9aad6079cad88425de6bde1a9187ebb6092cf67bf2b13fd65f270"
     "88d78b7e883c8759d2c4f5c65adb7553878ad575f9fad878e80a0c9ba63bcbcc2732e69485bbc9c90bfbd62481d9089b"
     "eccf80cfe2df16a2cf65bd92dd597b0707e0917af48bbb75fed413d238f5555a7a569d80c3414a8d0859dc65a46128ba"
     "b27af87a71314f318c782b23ebfe808b82b0ce26401d2e22f04d83d1255dc51addd3b75a2b1ae0784504df543af8969b"
     "e3ea7082ff7fc9888c144da2af58429ec96031dbcad3dad9af0dcbaaaf268cb8fcffead94f3c7ca495e056a9b47acdb7"
     "51fb73e666c6c655ade8297297d07ad1ba5e43f1bca32301651339e22904cc8c42f58c30c04aafdb038dda0847dd988d"
     "cda6f3bfd15c4b4c4525004aa06eeff8ca61783aacec57fb3d1f92b0fe2fd1a85f6724517b65e614ad6808d6f6ee34df"
     "f7310fdc82aebfd904b01e1dc54b2927094b2db68d6f903b68401adebf5a7e08d78ff4ef5d63653a65040cf9bfd4aca7"
     "984a74d37145986780fc0b16ac451649de6188a7dbdf191f64b5fc5e2ab47b57f7f7276cd419c17a3ca8e1b939ae49e4"
     "88acba6b965610b5480109c8b17b80e1b7b750dfc7598d5d5011fd2dcc5600a32ef5b52a1ecc820e308aa342721aac09"
     "43bf6686b64b2579376504ccc493d97e6aed3fb0f9cd71a43dd497f01f17c0e2cb3797aa2a2f256656168e6c496afc5f"
     "b93246f6b1116398a346f1a641f3b041e989f7914f90cc2c7fff357876e506b50d334ba77c225bc307ba537152f3f161"
     "0e4eafe595f6d9d90d11faa933a15ef1369546868a7f3a45a96768d40fd9d03412c091c6315cf4fde7cb68606937380d"
     "b2eaaa707b4c4185c32eddcdd306705e4dc1ffc872eeee475a64dfac86aba41c0618983f8741c5ef68d3a101e8a3b8ca"
     "c60c905c15fc910840b94c00a0b9d0",
     "0aab4c900501b3e24d7cdf4663326a3a87df5e4843b2cbdb67cbf6e460fec350"
     "aa5371b1508f9f4528ecea23c436d94b5e8fcd4f681e30a6ac00a9704a188a03"),
]
# the lengths at which prefix || M (32 + len) and R || A || M (64 + len) cross a SHA-512 block, and beyond
LENGTHS = [0, 1, 32, 47, 48, 79, 80, 143, 144, 175, 176, 300, 1023]
SEEDS = [E.entropy_to_seed(20), bytes.fromhex(RFC8032[2][0])]


@pytest.fixture(scope="module")
def sign_harness():
    """tests/sign_harness.cpp built as conftest.py builds host_harness.cpp."""
    lib = os.path.join(REPO, "tests", "_build", "libcvsign.so")
    src = os.path.join(REPO, "tests", "sign_harness.cpp")
    csrc = os.path.join(REPO, "corda_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
        os.makedirs(os.path.dirname(lib), exist_ok=True)
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-DCV_BOUNDS_CHECK", "-fPIC",
                        "-shared", src, "-o", lib], check=True)
    h = ctypes.CDLL(lib)
    h.cvs_bw16_built.restype = ctypes.c_size_t
    return h


def _mul_base_w16(h, k: int) -> bytes:
    out = ctypes.create_string_buffer(32)
    h.cvs_scalarmult_base_w16(k.to_bytes(32, "little"), out)
    return out.raw


def _expand(h, seed: bytes):
    a, prefix, abyte = (ctypes.create_string_buffer(32) for _ in range(3))
    h.cvs_key_expand(seed, a, prefix, abyte)
    return a.raw, prefix.raw, abyte.raw


def _sign(h, seed: bytes, msg: bytes) -> bytes:
    a, prefix, abyte = _expand(h, seed)
    sig = ctypes.create_string_buffer(64)
    h.cvs_sign_keyed(a, prefix, abyte, msg, len(msg), sig)
    return sig.raw


def _digits(d: int) -> int:
    """The scalar whose sixteen 16-bit digits are all d, cut below bit 253 (the procedure's domain)."""
    return sum(d << (16 * i) for i in range(16)) & ((1 << 253) - 1)


def test_scalarmult_base_w16_edges(sign_harness):
    """k = 0, 1, 2, L - 1, 2^252, 2^253 - 1 and the digit patterns that drive the recoding's carry chain: all
    0x7fff (no carry, the largest positive digits), all 0x8000 (every digit -32,768: the rows' last entry, a carry
    into every next digit), all 0xffff below bit 253 (= 2^253 - 1: a carry through every digit into the top one)."""
    ks = [0, 1, 2, E.L - 1, 1 << 252, (1 << 253) - 1, _digits(0x7fff), _digits(0x8000), _digits(0xffff)]
    assert ks[-1] == (1 << 253) - 1
    for k in ks:
        assert _mul_base_w16(sign_harness, k) == E.pt_encode(E.pt_mul(k, E.BASE)), hex(k)


def test_scalarmult_base_w16_random(sign_harness):
    rng = np.random.default_rng(8032)
    for _ in range(200):
        k = int.from_bytes(rng.bytes(40), "little") % E.L
        assert _mul_base_w16(sign_harness, k) == E.pt_encode(E.pt_mul(k, E.BASE)), hex(k)
    # the table is filled on demand: 16 entries per scalar at the most, of 4 x 32,769
    assert sign_harness.cvs_bw16_built() <= 16 * 400


def test_key_expand(sign_harness):
    rng = np.random.default_rng(20)
    seeds = [bytes.fromhex(v[0]) for v in RFC8032] + [E.entropy_to_seed(20), E.entropy_to_seed(10)]
    seeds += [rng.bytes(32) for _ in range(32)]
    for seed in seeds:
        a, prefix, abyte = _expand(sign_harness, seed)
        wa, wprefix, wabyte = E.seed_to_keypair(seed)
        assert (int.from_bytes(a, "little"), prefix, abyte) == (wa, wprefix, wabyte), seed.hex()
        assert abyte == E.public_key_of(seed)
    for seed, pk, _, _ in RFC8032:
        assert _expand(sign_harness, bytes.fromhex(seed))[2] == bytes.fromhex(pk)


@pytest.mark.parametrize("which", range(len(SEEDS)))
def test_sign_keyed_one_lengths(sign_harness, which):
    seed = SEEDS[which]
    rng = np.random.default_rng(100 + which)
    for n in LENGTHS:
        msg = rng.bytes(n)
        assert _sign(sign_harness, seed, msg) == E.sign(seed, msg), n


def test_sign_keyed_one_unaligned_message(sign_harness):
    """The hash reads the message in aligned words: every start alignment gives the same signature."""
    seed = SEEDS[0]
    body = np.random.default_rng(3).bytes(200)
    a, prefix, abyte = _expand(sign_harness, seed)
    for shift in range(4):
        buf = ctypes.create_string_buffer(b"\xee" * shift + body + b"\xee" * 8)
        sig = ctypes.create_string_buffer(64)
        sign_harness.cvs_sign_keyed(a, prefix, abyte, ctypes.byref(buf, shift), 143, sig)
        assert sig.raw == E.sign(seed, body[:143]), shift


def test_null_context_and_signer_rejected():
    """The C-ABI guards that need no device: a null context or signer is CV_E_ARGS, closing NULL is a no-op."""
    from corda_amd import native
    lib = native.load()
    out = ctypes.c_void_p(1)
    assert lib.cv_signer_open(None, bytes(32), ctypes.byref(out)) == -3 and not out.value
    assert lib.cv_signer_public_key(None, None) == -3
    assert lib.cv_signer_close(None) is None
    assert lib.cv_ed25519_sign_keyed(None, None, 1, None, 0, None, None, None) == -3
    assert lib.cv_ed25519_sign_keyed_device(None, 0, None, 1, None, None, None, None, None) == -3


def test_sign_keyed_one_rfc8032(sign_harness):
    """RFC 8032 section 7.1: tests 1-3, the 1,023-byte test and SHA(abc), published signatures as literals."""
    assert [len(v[2]) // 2 for v in RFC8032] == [0, 1, 2, 64, 1023]
    for seed, pk, msg, sig in RFC8032:
        assert _sign(sign_harness, bytes.fromhex(seed), bytes.fromhex(msg)) == bytes.fromhex(sig)
        assert E.sign(bytes.fromhex(seed), bytes.fromhex(msg)) == bytes.fromhex(sig)
