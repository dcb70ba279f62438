#!/usr/bin/env python
"""Record the bits of the K-split BPTT sweep for tests/test_gpu_rnn_seq_bwd_ring.py: sha256 of dZ (both directions) and of both bias sums
for that file's GOLDEN_CASES, on the inputs of tests/rnn_seq_ref.make_inputs.  Run it on the commit whose kernel is the yardstick:

    python tools/record_bptt_bits.py [out.json]        (default: tests/golden/bptt_bits_parent.json)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "automatic-speech-recognition_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import test_gpu_rnn_seq_bwd_ring as ring
    out = sys.argv[1] if len(sys.argv) > 1 else ring.GOLDEN
    cases = {ring.case_id(c): ring.result_bits(ring.swept(c)) for c in ring.GOLDEN_CASES}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump({"what": "sha256 of dZ [B, T, G H] bf16 per direction and of the bias sums (float64 of the fp32 sums minus DB_INIT)",
                   "cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d cases to %s" % (len(cases), out))


if __name__ == "__main__":
    main()
