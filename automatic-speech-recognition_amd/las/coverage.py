"""las.coverage -- attention coverage of the beam search's hypotheses: the host side.  The setting the flags ask for
(`from_args`, `Setting`), the counts of finished alignments (`rows_counts`: las_coverage_rows) and the fields of a JSON record
(`fields`).  The per-step scorer is las.beam_step.CoverageScorer (las_coverage_step, csrc/coverage.hip)."""
import collections

import numpy as np

Setting = collections.namedtuple("Setting", "w_c w_o tau kappa report")

FLAGS = ("--coverage_weight", "--overattend_weight", "--coverage_threshold", "--overattend_threshold", "--coverage_report")


def make(w_c=0.0, w_o=0.0, tau=0.5, kappa=1.5, report=False, what="set_coverage"):
    """the checked Setting, or None when nothing asks for the scorer (both weights 0 and no report).  Refused: a negative or
    non-finite weight, tau <= 0, kappa <= tau (or a threshold that is not finite)"""
    w_c, w_o, tau, kappa = (float(x) for x in (w_c, w_o, tau, kappa))
    for name, w in (("coverage", w_c), ("overattend", w_o)):
        if not np.isfinite(w) or w < 0 or np.float32(w) > np.float32(3.0e38):
            raise ValueError("%s: the %s weight must be finite and >= 0 (got %r)" % (what, name, w))
    if not (np.isfinite(tau) and np.float32(tau) > 0):
        raise ValueError("%s: the coverage threshold must be finite and > 0 (got %r)" % (what, tau))
    if not (np.isfinite(kappa) and np.float32(kappa) > np.float32(tau)):
        raise ValueError("%s: the over-attention threshold must be finite and above the coverage threshold %r (got %r)" % (what, tau, kappa))
    if w_c == 0 and w_o == 0 and not report:
        return None
    return Setting(w_c, w_o, tau, kappa, bool(report))


def from_args(args):
    """the Setting --coverage_weight / --overattend_weight / --coverage_threshold / --overattend_threshold / --coverage_report ask
    for, or None (all off).  Every flag is read with its default: a namespace from before these flags passes."""
    return make(getattr(args, "coverage_weight", 0.0) or 0.0, getattr(args, "overattend_weight", 0.0) or 0.0,
                getattr(args, "coverage_threshold", 0.5), getattr(args, "overattend_threshold", 1.5),
                bool(getattr(args, "coverage_report", False)), what="--coverage_* / --overattend_*")


def requested(args):
    """whether the flags switch the scorer on (a non-zero weight or a report); thresholds alone do not"""
    return bool(float(getattr(args, "coverage_weight", 0.0) or 0.0) != 0.0 or float(getattr(args, "overattend_weight", 0.0) or 0.0) != 0.0 or
                getattr(args, "coverage_report", False))


def refuse_without_attention(args, mode):
    """the modes that run no attention decoder (--decoder ctc without --rescore attention, --keywords, --align_text): a weight or a
    report there is a ValueError"""
    if requested(args):
        raise ValueError("%s runs no attention decoder: --coverage_weight / --overattend_weight / --coverage_report have nothing to "
                         "count there" % mode)


def frames_of(enc_len, Tp):
    """T'_u as the kernels clamp it"""
    return min(max(int(enc_len), 0), int(Tp))


def rows_counts(alphas, steps, enc_len, tau, kappa):
    """las_coverage_rows: alphas fp32 [U, R, Tp] on the device (the teacher-forced Speller's layout), steps / enc_len int per row ->
    int32 [R, 2] (covered, over) on the device"""
    import torch
    from las import _hip
    _hip.require_gpu(alphas)
    alphas = alphas.contiguous()
    U, R, Tp = alphas.shape
    i32 = dict(dtype=torch.int32, device=alphas.device)
    st = torch.as_tensor(np.asarray(steps, np.int64).reshape(-1)).to(**i32) if not torch.is_tensor(steps) else steps.to(**i32)
    el = torch.as_tensor(np.asarray(enc_len, np.int64).reshape(-1)).to(**i32) if not torch.is_tensor(enc_len) else enc_len.to(**i32)
    if st.numel() != R or el.numel() != R:
        raise ValueError("rows_counts: %d rows, %d step counts, %d lengths" % (R, st.numel(), el.numel()))
    counts = torch.zeros(R, 2, **i32)
    _hip.check(_hip.lib().las_coverage_rows(_hip.p(alphas), U, R, Tp, _hip.p(st), _hip.p(el), float(tau), float(kappa), _hip.p(counts),
                                            _hip.stream()), "las_coverage_rows")
    return counts


def gain_total(setting, covered, over):
    """a finished hypothesis' whole coverage term as the second pass adds it: fl32(fl32(w_c covered) - fl32(w_o over))"""
    f = np.float32
    return f(f(f(setting.w_c) * f(covered)) - f(f(setting.w_o) * f(over)))


def fields(cov):
    """the JSON fields of a hypothesis' (covered, over, frames): shares of its utterance's encoder frames ({} without counts)"""
    if cov is None:
        return {}
    covered, over, frames = cov
    d = max(int(frames), 1)
    return {"coverage": round(int(covered) / d, 4), "overattended": round(int(over) / d, 4)}
