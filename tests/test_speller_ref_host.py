"""Without a GPU: the bound tests/test_gpu_speller_rnn_cell.py holds the Speller's bf16 families to can tell a wrong kernel from a right one.

For both cells and one small shape per class (additive T' <= 128, additive T' = 160, mixed sampling, location-aware K = 201 / C = 10, two
layers), every mutation of speller_ref.MUTATIONS -- the smallest realistic kernel mistakes, stated as edits of the oracle's inputs -- moves the
oracle's logits, and every gradient tensor it can reach, by MORE than bound(floor) = MARGIN x the oracle's own flip floor on the same inputs.
And every shape of the GPU table has a floor that is non-zero and below 2e-2: at 2e-2, MARGIN x floor would reach the smallest mutation's
error on the slowest-moving tensors (2.5e-2) and the shape could not discriminate.

Measured (error / bound, the smallest over logits and the reachable gradients; MARGIN = 4): tanh cell 1.21 (one k-row zeroed, location-aware,
on conv1d/kernel) and 1.26 (one k-row, two layers, on the embedding) .. 33; LSTM 1.39 (one k-row, mixed sampling, on the cell kernel) .. 35.  On
the logits alone: at least 1.9 (tanh cell) and 2.8 (LSTM).  The largest floor of a GPU-table shape is 1.2e-2 (a gradient tensor at T' = 160)."""
import pytest

import helpers  # noqa: F401  (sys.path)
import speller_ref as SR
import test_gpu_speller_rnn_cell as GT

CLASSES = {
    "add_le128": (1, 512, 128, 256, 5, 37, 9, False, None),
    "add_160": (1, 512, 128, 256, 4, 160, 6, False, None),
    "mixed": (1, 512, 128, 256, 3, 131, 5, True, None),
    "loc": (1, 512, 128, 256, 5, 37, 9, False, (201, 10)),
    "two_layers": (2, 64, 32, 64, 4, 21, 7, True, None),
}


def _compared(fl):
    """the quantities the condition is about: logits and every gradient tensor, in relative L2"""
    return [k for k in fl if k == "logits" or k.startswith("grad/")]


@pytest.mark.parametrize("cell", ["rnn", "lstm"])
@pytest.mark.parametrize("cname", sorted(CLASSES))
def test_every_mutation_exceeds_the_bound(cname, cell):
    shape = CLASSES[cname]
    seen = 0
    for name, (applies, _, _, excused) in SR.MUTATIONS.items():
        if not applies(cell, shape):
            continue
        seen += 1
        err, fl = SR.mutation_errors(cell, shape, name)
        bnd = SR.bound(fl)
        skip = dict(SR.UNREACHABLE, **excused)
        assert fl["grad/" + SR.VOCAB_B] == 0 and err["grad/" + SR.VOCAB_B] == 0        # the reason it is out: 0 / 0
        must = [k for k in _compared(fl) if k[5:] not in skip]
        assert "logits" in must and len(must) >= len(_compared(fl)) - 3
        ratios = {k: err[k] / bnd[k] for k in must}
        low = min(ratios, key=ratios.get)
        print("MUTATION %s %s %s: logits %.1f x the bound, smallest %s %.2f x" % (cname, cell, name, ratios["logits"], low, ratios[low]))
        for k in must:
            assert fl[k] > 0, (name, k)
            assert err[k] > bnd[k], (cname, cell, name, k, err[k], bnd[k])
    assert seen >= 6 + int(shape[7]) + 2 * int(shape[8] is not None)          # no mutation left out


def _table_cases():
    cases = {(row[0], GT.row_rows(row), None) for row in GT.ROWS}
    cases.add((GT.T37, "bf", "short"))
    return sorted(cases, key=str)


@pytest.mark.parametrize("case", _table_cases(), ids=lambda c: "-".join(str(x) for x in c[0][:8]) + "-%s-%s" % (c[1], c[2]))
def test_gpu_table_floor_is_nonzero_and_discriminates(case):
    shape, rows, variant = case
    fl = SR.floor_of("rnn", shape, rows, variant)
    print("FLOOR %s %s %s: logits %.1e alphas %.1e gradients %.1e max-norm %.1e" % (
        shape, rows, variant, fl["logits"], fl["alphas"], max(fl[k] for k in fl if k.startswith("grad/")), max(fl[k] for k in fl if "max" in k)))
    for k, v in fl.items():
        if k in ("grad/" + SR.VOCAB_B, "gmax/" + SR.VOCAB_B):
            assert v == 0, (k, v)
            continue
        assert v > 0, (k, v)
        if "max" not in k:
            assert v < 2e-2, (k, v)


def test_the_gpu_table_names_what_it_has_to():
    fams = {p: set() for p in (2, 3)}
    for row in GT.ROWS:
        for p in (2, 3):
            fams[p] |= set(row[p])
    for p in (2, 3):
        assert {"loop", "pf_rows", "bf_rows", "f32_rows", "loc"} <= fams[p], fams[p]
    loops = [r for r in GT.ROWS if "loop" in r[2] and not r[1]]
    assert {8, 10, 12, 14} <= {8 if r[0][5] <= 128 else 10 if r[0][5] <= 160 else 12 if r[0][5] <= 192 else 14 for r in loops}
    assert max((r[0][4] + 7) // 8 for r in loops) == 16                       # R = 16 row workgroups per group
    assert len(GT.ROWS) + 3 <= 40
    assert len({GT.row_id(r) for r in GT.ROWS}) == len(GT.ROWS)
