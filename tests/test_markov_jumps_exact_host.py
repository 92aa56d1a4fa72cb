"""The exact yardstick of the Markov-jump and robust-count tables (tests/markov_jumps_exact.py), CPU tier: the yardstick against
mpmath at 50 digits; the two host restatements (tests/markov_jumps_reference.py, tests/robust_counting_reference.py) against the
yardstick on every case the GPU tier (tests/test_gpu_markov_jumps_exact.py) runs; the checker rejecting five wrong restatements; and
the gather's expected coverage.  Run with -s for the figures DESIGN.md section 6 tabulates.

Measured here (worst metric value per regime over its cases and registers; DESIGN.md section 6 has every row):
  yardstick against mpmath: 1.1e-18 at most (well 8.5e-19, tied 3.5e-19, near 1.1e-18, short 1.5e-19)
  restatement against yardstick: well 6.6e-11 (100 states, tau 0.05, the reward register; 6.6e-13 at tau 1, 2.0e-15 at tau 30),
  tied 7.0e-14, thin 6.2e-10, near 6.4e-9 (a gap under the tie threshold at tau 1; 2.9e-11 just above it), short 1.4e-8 at tau
  1e-3, 2.3e-2 at 1e-6 and 84 at 1e-8 in the reward register (counts: 1.3e-10, 1.3e-7, 1.2e-5); robust counts 3.3e-13 at
  tau >= 0.3, 1.3e-11 at 0.4 on the general register, 1.2e-7 on the near-tie chain, 0.11 on a branch of 1e-6
"""
import numpy as np
import pytest

import markov_jumps_exact as mx
import markov_jumps_reference as mr

JUMP_CASES = mx.host_jump_cases()
WELL = [c for c in JUMP_CASES if c.regime == "well"]
HARD_BOUND = ("well", "tied")


def worst_over_table(case, candidate):
    """-> (worst of the candidate, worst of the restatement, bound), each per register, over the whole table of the case."""
    U, Ui, lam, cond, unit = mx.host_tables(case)
    return mx.judge(case.regime, candidate, case.restatement(U, Ui, lam), cond, unit[:, :, None, None])


@pytest.mark.parametrize("case", [c for c in JUMP_CASES if c.mpmath], ids=repr)
def test_yardstick_against_mpmath(case):
    """The long double block exponential against mpmath's at 50 digits: at most 1e-13 in the metric (1000 x inside the project's
    bound), and where the restatement's own loss is the bound (near-tie, short), at least 100 x below that loss."""
    pytest.importorskip("mpmath")
    U, Ui, lam, cond, unit = mx.host_tables(case)
    mp = mx.mpmath_cond(U, Ui, lam, case.registers, case.kinds, case.scale_by_time, case.time, case.branch_rate, case.cat_rates)
    yard = mx.metric_against_mpmath(cond, unit, mp)
    _, rest, _ = worst_over_table(case, case.restatement(U, Ui, lam))
    print("%s (%s): yardstick vs mpmath %s; restatement vs yardstick %s" % (
        case.name, case.regime, " ".join("%.1e" % y for y in yard), " ".join("%.1e" % r for r in rest)))
    assert np.all(yard <= 1e-13), yard
    if case.regime not in HARD_BOUND:
        assert np.all(100.0 * yard <= rest), (yard, rest)


@pytest.mark.parametrize("case", JUMP_CASES, ids=repr)
def test_markov_jump_restatement_against_the_yardstick(case):
    U, Ui, lam, _, _ = mx.host_tables(case)
    _, rest, _ = worst_over_table(case, case.restatement(U, Ui, lam))
    print("%s (%s) restatement vs yardstick: %s" % (case.name, case.regime, " ".join(
        "%s %.2e" % (t, r) for t, r in zip(case.tags, rest))))
    assert np.all(np.isfinite(rest))
    if case.regime in HARD_BOUND:
        assert np.all(rest <= mx.BOUND), rest


@pytest.mark.parametrize("case", mx.robust_cases(), ids=repr)
def test_robust_count_restatement_against_the_yardstick(case):
    """Every 64 x 64 table of every branch; a row is judged by its own regime (a branch of 1e-3 or less is a short one)."""
    lengths = case.branch_lengths()
    taus = np.concatenate([[0.0], np.unique(lengths[lengths > 0.0])])
    exact, rest, mask = case.exact(taus), case.restatement(taus), case.resolvable(taus)
    for r in range(1, len(taus)):
        regime = case.row_regime(taus[r])
        _, worst, _ = mx.judge(regime, rest[:, r], rest[:, r], exact[:, r], case.units()[:, None, None], mask[r])
        assert np.all(np.isfinite(rest[:, r][:, mask[r]]))
        print("%s tau %g (%s) restatement vs yardstick: %s; %.1f %% of the entries below float64's resolution of P" % (
            case.name, taus[r], regime, " ".join("%.2e" % w for w in worst), 100.0 * (1.0 - mask[r].mean())))
        if regime in HARD_BOUND:
            assert mask[r].all() and np.all(worst <= mx.BOUND), (taus[r], worst)


def m_from_the_wrong_side(U, Ui, rate_reg):
    return mr.mm(U, mr.mm(rate_reg, Ui))


def tie_branch(threshold, halved):
    def aux_int(lam, tau):
        tau = np.asarray(tau, dtype=np.float64)[..., None, None]
        e = np.exp(lam[None, :] * tau)
        ea, eb = np.swapaxes(e, -1, -2), e
        la, lb = lam[:, None], lam[None, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(np.abs(la - lb) < threshold, eb * tau / 2.0 if halved else ea * tau, (ea - eb) / (la - lb))
    return aux_int


def perturbed(case, which, monkeypatch):
    """The restatement's tables with one thing wrong."""
    U, Ui, lam, _, _ = mx.host_tables(case)
    tau = (case.time * case.branch_rate) * case.cat_rates
    P = mr.mm(U, np.exp(lam[None, :] * tau[:, None])[:, :, None] * Ui)
    if which == "M = U R U^-1":
        monkeypatch.setattr(mr, "precompute", m_from_the_wrong_side)
    elif which == "tie branch eb tau / 2":
        monkeypatch.setattr(mr, "aux_int", tie_branch(1e-7, True))
    elif which == "tie threshold 1e-5":
        monkeypatch.setattr(mr, "aux_int", tie_branch(1e-5, False))
    if which == "P transposed":
        return case.restatement(U, Ui, lam, matrices=np.swapaxes(P, -1, -2))
    if which == "scale_by_time dropped":
        return case.restatement(U, Ui, lam, scale_by_time=[False] * len(case.registers))
    return case.restatement(U, Ui, lam)


@pytest.mark.parametrize("which", ["M = U R U^-1", "P transposed", "scale_by_time dropped", "tie branch eb tau / 2"])
@pytest.mark.parametrize("case", WELL, ids=repr)
def test_the_checker_rejects_a_wrong_restatement(case, which, monkeypatch):
    wrong = perturbed(case, which, monkeypatch)
    monkeypatch.undo()
    got, _, bound = worst_over_table(case, wrong)
    print("%s, %s: %s against %s" % (case.name, which, got, bound))
    assert np.any(got > bound), (got, bound)
    if which != "scale_by_time dropped":
        assert np.all(got > bound), (got, bound)                  # every register notices (the first is not scaled by time)


@pytest.mark.parametrize("case", [c for c in JUMP_CASES if c.name.startswith("hky-d1e-05")], ids=repr)
def test_the_checker_rejects_a_tie_threshold_of_1e_5(case, monkeypatch):
    wrong = perturbed(case, "tie threshold 1e-5", monkeypatch)
    monkeypatch.undo()
    got, rest, bound = worst_over_table(case, wrong)
    print("%s: %s against %s (restatement %s)" % (case.name, got, bound, rest))
    assert np.all(got > bound), (got, bound)


@pytest.mark.parametrize("case", mx.jump_cases(), ids=repr)
def test_expected_coverage_of_the_gather(case):
    """From the model alone: at most 0.1 % of a row's table entries are expected to go ungathered, and the patterns cross a
    256-pattern workgroup."""
    host = next(c for c in JUMP_CASES if c.name == case.name.replace("-device", "")) if case.device_eigen else case
    U, Ui, lam = mx.host_tables(host)[:3]
    R = mx.host_repeats(host)
    share = mx.expected_missing_share(case, mx.exact_p(host, U, Ui, lam), R)
    print("%s: R = %d, %d patterns, expected share never gathered %.2e" % (case.name, R, R * case.S ** 2, share))
    assert R * case.S ** 2 > 256 and share <= mx.COVERAGE_EXPECTED
