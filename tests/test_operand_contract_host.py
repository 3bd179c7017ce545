"""The operand-contract table (tests/helpers/operand_contract.py) on the host: every route has cases, every feature its
entry point accepts is exercised on every route, the refusals are asked everywhere, and every mutated reference -- what a
kernel that silently ignored a feature would produce -- misses the true reference by at least MUTATION_MARGIN bounds, so
each GPU case would catch its feature being dropped.  The mutation check runs each case's own input construction at a
reduced batch and grid (the same channels and features), which keeps the whole file to seconds."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import operand_contract as OC  # noqa: E402
import operand_contract_fused as FC  # noqa: E402

CASES = OC.all_cases()


def _small(case):
    """The case's batch (at most 3) on a small grid: wgrad S grids of 8 x 16 (the generic route's own 10 x 12), 8 x 8
    elsewhere."""
    r = OC.ROUTE[case.route]
    if r.entry == "wgrad":
        return min(case.B, 3), ((8, 16) if r.shape[4] >= 16 else (r.shape[3], r.shape[4]))
    return min(case.B, 3), (8, 8)


def test_every_route_has_cases_and_a_base_case():
    for r in OC.ROUTES:
        cs = OC.cases_for(r)
        assert cs, r.name
        assert any(c.feats == OC.normalize(r, ()) and c.expect == "match" for c in cs), r.name


def test_every_accepted_feature_is_exercised_on_every_route():
    for r in OC.ROUTES:
        seen = set().union(*(c.feats for c in OC.cases_for(r) if c.expect == "match"))
        want = OC.feature_axes()[r.entry] - set(OC.REFUSED[r.entry])
        if r.entry == "wgrad" and not OC.t_affine2_route(r):
            want.discard("tmode4")
        if r.entry == "s2" and r.shape[1] == 1:
            want.discard("ones")
        if "tmode4" in r.base:                    # T = AFFINE2: S plain or BatchNorm-applied, shared coefficients
            want = {"smode1", "smode2", "smode3", "sps", "tps", "tmode4"}
        if "border" in r.base:
            want.discard("bias")                  # the border table replaces the plain bias
        assert want <= seen, (r.name, sorted(want - seen))


def test_every_refusal_is_asked_on_every_route():
    for r in OC.ROUTES:
        refused = [c for c in OC.cases_for(r) if c.expect == "refuse"]
        for k in OC.REFUSED[r.entry]:
            assert any(k in c.feats for c in refused), (r.name, k)
    aff2 = OC.cases_for(OC.ROUTE["wg_wide1_t_affine2"])
    assert any(c.expect == "refuse" and "smode4" in c.feats for c in aff2)
    assert any(c.expect == "match" and "tps" in c.feats for c in aff2)
    assert any(c.expect == "match" and "sps" in c.feats for c in aff2)


def test_every_route_has_a_case_beyond_its_persistent_grid():
    """Every route but dm_apply has one case with more tile units than its grid can hold (by the dm_*_num_blocks formula),
    with per-sample coefficients wherever the route's kernel takes them."""
    for r in OC.ROUTES:
        if r.entry == "apply":
            continue
        big = [c for c in OC.cases_for(r) if c.B == OC.persistent_B(r)]
        assert len(big) == 1 and big[0].expect == "match", r.name
        units, cap = OC.declared_units(r, big[0].B)
        assert units > cap or "per_tile" in r.base, (r.name, units, cap)
        if OC.takes_per_sample(r) and "tmode4" not in r.base:
            assert big[0].feats & {"ps", "sps"}, r.name
        else:
            assert not big[0].feats & {"ps", "sps", "tps", "mask_aff_ps"}, r.name


def test_case_ids_are_unique():
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids))


@pytest.mark.parametrize("route", [r.name for r in OC.ROUTES])
def test_every_mutation_is_visible(route):
    for case in OC.cases_for(OC.ROUTE[route]):
        if case.expect != "match":
            continue
        B, hw = _small(case)
        X = OC.make_inputs(case, B=B, hw=hw)
        R = OC.reference(case, X)
        for mut in OC.mutations_of(case):
            r = OC.max_ratio(R, OC.reference(case, X, mut))
            assert r >= OC.MUTATION_MARGIN, f"{case.id}: mutation {mut} only {r:.1f} bounds from the reference"


def test_fused_backward_entries_have_their_dy_modes_and_refusals():
    for name, entry, _, _ in FC.FUSED_ROUTES:
        cs = FC.fused_cases()
        mine = [c for c in cs if c.route == name]
        if entry != "convt":
            assert {FC._dy_mode(c.feats) for c in mine if c.expect == "match"} == {0, 4}, name
            assert any("dy_ps" in c.feats and c.expect == "refuse" for c in mine), name
        assert any(c.expect == "match" for c in mine), name


def test_every_fused_mutation_is_visible():
    for case in FC.fused_cases():
        if case.expect != "match":
            continue
        X = FC.make_fused_inputs(case)
        R = FC.fused_reference(case, X)
        for mut in FC.fused_mutations(case):
            r = FC.fused_max_ratio(R, FC.fused_reference(case, X, mut))
            assert r >= OC.MUTATION_MARGIN, f"{case.id}: mutation {mut} only {r:.1f} bounds from the reference"
