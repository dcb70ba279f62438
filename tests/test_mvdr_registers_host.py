"""The MVDR kernels (csrc/mvdr.hip) hold the covariance pass's accumulators (up to 180 fp32 values a thread) and the solve's
sixteen complex doubles in registers.  That is a property of the build: the compiler's resource report of the shipped object
(csrc/build/mvdr.res, written by the Makefile) must show no scratch and no spilled vector register in ANY kernel of the file.  No GPU needed."""
import os
import re
import subprocess

import helpers  # noqa: F401  (sys.path)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "automatic-speech-recognition_amd", "csrc")
FIELDS = {"VGPRs": r"\bVGPRs: (\d+)", "scratch": r"ScratchSize \[bytes/lane\]: (\d+)", "sgpr_spill": r"SGPRs Spill: (\d+)",
          "vgpr_spill": r"VGPRs Spill: (\d+)", "lds": r"LDS Size \[bytes/block\]: (\d+)"}


def report():
    res = os.path.join(CSRC, "build", "mvdr.res")
    if not os.path.exists(res):                      # the report comes with the object: the Makefile's rule for build/mvdr.o writes both
        subprocess.check_call(["make", "-C", CSRC, "-B", "build/mvdr.o"], stdout=subprocess.DEVNULL)     # (-B: an object from an older Makefile)
    assert os.path.exists(res), "csrc/build/mvdr.o was not built by csrc/Makefile: no compiler report next to it (make clean; make)"
    cur, out = None, {}
    for line in open(res):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            out[cur] = {}
        for k, pat in FIELDS.items():
            m = re.search(pat, line)
            if m and cur:
                out[cur][k] = int(m.group(1))
    return out


def test_no_mvdr_kernel_uses_scratch_or_spills():
    rep = report()
    names = " ".join(rep)
    for kernel in ("fft_tables_kernel","mvdr_energy_kernel", "mvdr_max_kernel", "mvdr_mask_kernel", "mvdr_cov_kernel", "mvdr_counts_kernel",
                   "mvdr_n0_kernel", "mvdr_phi_y_kernel", "mvdr_phi_n_kernel", "mvdr_weights_kernel", "mvdr_hold_kernel", "mvdr_apply_kernel"):
        assert kernel in names, kernel
    assert len(rep) == 21                             # 8 instantiations of the covariance kernel, 2 each of the energy and apply kernels
    for name, r in rep.items():
        print("%-70s VGPRs %3d LDS %6d" % (name[:70], r["VGPRs"], r["lds"]))
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)    # (scalar registers parked in vector lanes cost no memory)
    cov = [r["VGPRs"] for name, r in rep.items() if "mvdr_cov_kernel" in name]
    assert max(cov) <= 256                            # a workgroup of 512 threads: 256 registers a thread
