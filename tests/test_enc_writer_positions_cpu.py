"""The multi-wave encoders' byte writer (StagedWriter::emit, csrc/rcx_mc.hpp) keeps its position as two running values
instead of recomputing them from pos8 = 8 x the bytes produced: np = 0 - pos8, moved by np -= k8, whose bits 3-4 are the
shift that brings the window's end up to a word boundary, and q = (pos8 - 40) << 3, moved by q += k8 << 3, whose bits 8-13
are the older word's slot of 256 bytes in a ring of 64, ORed into the lane's address in slot 0 -- right where the ring
begins at a multiple of 16 KiB.  Here as integer arithmetic with u32 wrap-around, for every position a 64 KiB block can
reach (and the stream's start, where pos8 - 40 is negative) and every step a symbol can make.  On the GPU against the
oracle: tests/test_gpu_enc_writer_positions.py.
"""
import numpy as np

U32 = np.uint32
RING_WORDS, LANES = 64, 64
SLOT_MASK = U32(0x3F00)
STEPS = (0, 8, 16, 24)          # k8: a symbol lets 0 to 3 bytes go
POS8 = (np.arange(1, 66001, dtype=np.uint64) * 8).astype(U32)
BASES = [U32(ring + 4 * lane) for ring in (0, 16384, 9 * 16384) for lane in (0, 1, 37, 63)]


def present_sh8(pos8):
    return (U32(0) - pos8) & U32(24)


def present_at(pos8, base):
    """ring_lane + (((pos8 - 40) >> 5) % 64) * RCX_LANES dwords, as a byte address"""
    return base + U32(256) * (((pos8 - U32(40)) >> U32(5)) % U32(RING_WORDS))


def running(pos8):
    return U32(0) - pos8, (pos8 - U32(40)) << U32(3)


def test_layout_constants():
    assert int(SLOT_MASK) == (RING_WORDS - 1) * LANES * 4 and RING_WORDS * LANES * 4 == 16384


def test_begin():
    """StagedWriter::begin: pos8 = 8 (the reference's initial zero byte), the older word in slot 63."""
    np_, q = running(np.array([8], U32))
    assert int(np_[0]) == 0xFFFFFFF8 and int(q[0]) == 0xFFFFFF00
    assert int(q[0] & SLOT_MASK) == 63 * 256


def test_running_values_at_every_position():
    with np.errstate(over="ignore"):
        np_, q = running(POS8)
        assert np.array_equal(np_ & U32(24), present_sh8(POS8))
        assert np.array_equal(U32(0) - np_, POS8)  # pos8 derived back for chunk_begins / finish / the carry paths
        for base in BASES:
            got = (q & SLOT_MASK) | base
            assert np.array_equal(got, present_at(POS8, base)), f"base {int(base):#x}"
            assert got.min() >= base and got.max() <= base + U32(63 * 256)


def test_every_step_from_every_position():
    """np -= k8 and q += k8 << 3 from every position give the values of pos8 + k8, and so the same shift and address."""
    with np.errstate(over="ignore"):
        np_, q = running(POS8)
        for k8 in STEPS:
            np2, q2 = np_ - U32(k8), q + (U32(k8) << U32(3))
            want_np, want_q = running(POS8 + U32(k8))
            assert np.array_equal(np2, want_np) and np.array_equal(q2, want_q), f"k8 {k8}"
            assert np.array_equal(np2 & U32(24), present_sh8(POS8 + U32(k8)))
            for base in BASES:
                assert np.array_equal((q2 & SLOT_MASK) | base, present_at(POS8 + U32(k8), base)), f"k8 {k8}, base {int(base):#x}"


def test_a_walk_of_steps():
    """The values as the writer carries them: from begin() through 200 000 symbols of random steps, never recomputed."""
    rs = np.random.RandomState(25)
    k8 = (8 * rs.randint(0, 4, 200000)).astype(U32)
    with np.errstate(over="ignore"):
        pos8 = U32(8) + np.concatenate([[0], np.cumsum(k8, dtype=U32)[:-1]]).astype(U32)
        np_ = U32(0xFFFFFFF8) - (pos8 - U32(8))
        q = U32(0xFFFFFF00) + ((pos8 - U32(8)) << U32(3))
        assert np.array_equal(np_ & U32(24), present_sh8(pos8))
        base = U32(16384 + 4 * 5)
        assert np.array_equal((q & SLOT_MASK) | base, present_at(pos8, base))


def test_identity_for_any_u32():
    """((x << 3) & 0x3F00) == (((x >> 5) & 63) << 8) for x around every wrap: the mask bounds the address whatever q holds."""
    rs = np.random.RandomState(26)
    x = np.concatenate([rs.randint(0, 1 << 32, 1 << 20, dtype=np.uint64), np.arange(1 << 12), (1 << 32) - 1 - np.arange(1 << 12),
                        (1 << 29) + np.arange(-2048, 2048)]).astype(U32)
    with np.errstate(over="ignore"):
        assert np.array_equal((x << U32(3)) & SLOT_MASK, ((x >> U32(5)) & U32(63)) << U32(8))
