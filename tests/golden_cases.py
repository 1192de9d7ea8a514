"""The generated inputs of the range-coder and rANS fixtures, label -> a callable that makes the bytes.  The makers under
tests/golden/ run the real reference over them and store the hash of every input with the reference's results; the tests
make them again from here and check that hash first."""
import numpy as np

from cpprcoder_amd import workloads

NO_HALVING = (1 << 24) - 256  # RCX_MAX_BLOCK: the longest stream whose table is never halved

# adaptive_static_kat.json "generated" (make_golden.py)
GENERATED = {
    "A*65535": lambda: b"A" * 65535, "A*65536": lambda: b"A" * 65536, "A*65537": lambda: b"A" * 65537,
    "ff*70000": lambda: b"\xff" * 70000,
    "uniform(65536,12345)": lambda: workloads.uniform(65536, 12345).tobytes(),
    "uniform(100000,7)": lambda: workloads.uniform(100000, 7).tobytes(),
    "zipf(65536,12345)": lambda: workloads.zipf(65536, 12345).tobytes(),
    "runs(200000,7)": lambda: workloads.runs(200000, 7).tobytes(),
}

# long_streams.json "adaptive" and "static" (make_golden_long.py): past 1 MiB, up to and through the halving at total = 2^24
LONG_ADAPTIVE = {
    "uniform(2MiB+77,3)": lambda: workloads.uniform((2 << 20) + 77, 3),
    "zipf(NO_HALVING,4)": lambda: workloads.zipf(NO_HALVING, 4),
    "uniform(NO_HALVING+5000,11)": lambda: workloads.uniform(NO_HALVING + 5000, 11),
    "min(zipf(2^24+70000,5),3)": lambda: np.minimum(workloads.zipf((1 << 24) + 70000, 5), 3).astype(np.uint8),
}
LONG_STATIC = {
    "zipf(2^24+1000,6)": lambda: workloads.zipf((1 << 24) + 1000, 6),
    "runs(3MiB,2)": lambda: workloads.runs(3 << 20, 2),
}

# rans.json "generated" (make_golden_rans.py)
RANS_GENERATED = {
    "A*65536": lambda: np.full(65536, 65, np.uint8),          # one symbol: encode_simd spends a word per symbol (cppans.h:357 wraps)
    "uniform(65536,12345)": lambda: workloads.uniform(65536, 12345),
    "uniform(100003,7)": lambda: workloads.uniform(100003, 7),
    "zipf(65536,12345)": lambda: workloads.zipf(65536, 12345),
    "runs(200000,7)": lambda: workloads.runs(200000, 7),
    "two symbols 1:70000": lambda: np.concatenate([np.zeros(70000, np.uint8), np.ones(1, np.uint8)]),  # the steal loop of normalize()
    "rare tail": lambda: np.concatenate([workloads.zipf(300000, 3), np.arange(256, dtype=np.uint8)]),
}
