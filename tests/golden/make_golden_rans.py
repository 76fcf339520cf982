"""Emit tests/golden/rans64_ref.npz: the streams the reference's vendored rans64.h writes for the escape-free problems
of tests/test_rans_codec.py::test_state_machine_equals_the_reference_header, through oracle/_ref/librans64_ref.so
(built by oracle/build_ref.sh where the reference is present).  Per problem t: cdf_t (uint32), sym_t (int16) and
words_t (uint32, the reference encoder's output).  Usage: python tests/golden/make_golden_rans.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..", "..")
for p in (ROOT, os.path.join(ROOT, "image-compression-for-machine_amd"), os.path.join(HERE, "..")):
    sys.path.insert(0, p)
import test_rans_codec as T  # noqa: E402


def main():
    if not os.path.exists(T.REF_SO):
        sys.exit(f"{T.REF_SO} not built: run oracle/build_ref.sh where the reference is present")
    encode, decode = T._ref_header()
    out = {}
    for t, (cdf, sym) in enumerate(T._header_cases()):
        words = encode(cdf, sym)
        assert decode(words, cdf, len(sym)) == (0, sym.tolist())
        out[f"cdf_{t}"] = cdf
        out[f"sym_{t}"] = sym.astype(np.int16)
        out[f"words_{t}"] = np.frombuffer(words, dtype=np.uint32)
    np.savez_compressed(os.path.join(HERE, "rans64_ref.npz"), **out)
    print("wrote", len(out) // 3, "problems")


if __name__ == "__main__":
    main()
