"""Every route behind dm_conv4x4s2, dm_conv3x3, dm_wgrad and dm_apply against the operand / epilogue contract of
include/dynamorph_hip.h (tests/helpers/operand_contract.py): each case either matches the float64 reference within the
accumulation bound -- output and statistics, no NaN pre-fill left in anything declared, the slab past the declared ones
untouched -- or is refused before any launch, exactly as the table says.  rc 0 with a wrong result fails.

The routes the streaming and one-pass kernels shadow run in ONE child process with DM_WIDE_STREAM=0 DM_WIDE_WGRAD1=0 (the
switches are read once per process)."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import operand_contract as OC  # noqa: E402
import operand_contract_fused as FC  # noqa: E402

pytestmark = pytest.mark.gpu

LOCAL = OC.all_cases("")
TILED = OC.all_cases("tiled")
FUSED = FC.fused_cases()


@pytest.mark.parametrize("case", LOCAL, ids=[c.id for c in LOCAL])
def test_route_honours_or_refuses(case):
    import operand_contract_run as RUN
    ok, msg = RUN.run_case(case)
    assert ok, f"{case.id}: {msg}"


@pytest.fixture(scope="module")
def tiled_results(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("contract") / "tiled.json")
    env = dict(os.environ, **OC.TILED_ENV)
    p = subprocess.run([sys.executable, os.path.join(HERE, "helpers", "operand_contract_run.py"), "tiled", out], env=env,
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, f"child exited {p.returncode}:\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    with open(out) as fh:
        return json.load(fh)


@pytest.mark.parametrize("case", TILED, ids=[c.id for c in TILED])
def test_tiled_route_honours_or_refuses(case, tiled_results):
    ok, msg = tiled_results[case.id]
    assert ok, f"{case.id} (DM_WIDE_STREAM=0 DM_WIDE_WGRAD1=0): {msg}"


@pytest.mark.parametrize("case", FUSED, ids=[c.id for c in FUSED])
def test_fused_backward_honours_or_refuses(case):
    import operand_contract_run as RUN
    ok, msg = RUN.run_fused(case)
    assert ok, f"{case.id}: {msg}"
