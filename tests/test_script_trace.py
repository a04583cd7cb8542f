"""CPU: the reference's runner scripts (tests/micro_*.sh, benchmark/micro_*.sh) are executed UNMODIFIED, as scripts, against recording
stubs (tests/ref_harness/trace_scripts.py); the GPU suite replays what they executed. Only where the reference tree exists."""
import json
import os
import sys
from pathlib import Path

import pytest

HARNESS = Path(__file__).resolve().parent / "ref_harness"
REF = Path("/root/reference")


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree not present (or not readable) on this box")
def test_reference_scripts_run_unmodified_and_trace(tmp_path):
    sys.path.insert(0, str(HARNESS))
    import trace_scripts
    out = tmp_path / "trace.json"
    assert trace_scripts.trace(REF, out) == 0
    t = json.loads(out.read_text())
    # every runner script of the reference was run, in its own directory's terms, and called at least one known binary
    assert sorted(t["scripts"]) == sorted(str(p.relative_to(REF)) for p in list(REF.glob("tests/micro_*.sh")) + list(REF.glob("benchmark/micro_*.sh")))
    by = {}
    for e in t["invocations"]:
        by.setdefault(e["script"], []).append(e)
        assert e["env"].get("FPGA_BITSTREAM", "").startswith("/nonexistent-bitstreams/")      # bitstream_dir.sh was sourced
        assert "FPGA_KERNEL" in e["env"]
    # spot checks against the scripts' own command lines (micro_keyswitch.sh:20-34, benchmark/micro_keyswitch.sh)
    ks = [(e["env"].get("N"), e["env"].get("BATCH_SIZE_KEYSWITCH")) for e in by["tests/micro_keyswitch.sh"]]
    assert ks == [(None, None), ("16384", "1"), ("16384", "2"), ("8192", "1"), ("8192", "1")]
    bk = [(e["env"]["ITER"], e["env"]["BATCH_SIZE_KEYSWITCH"]) for e in by["benchmark/micro_keyswitch.sh"]]
    assert bk == [("256", "1"), ("256", "16"), ("256", "128")]


def test_stub_ignores_what_its_own_interpreter_start_up_sets(tmp_path):
    """a start-up hook of the stub's python3 that sets a variable to another value in every process -- the first equal to the tracer's
    own, as can happen to the calibration run -- leaves no mark in what the stub records; what the caller sets is recorded"""
    import stat
    import subprocess
    sys.path.insert(0, str(HARNESS))
    import trace_scripts
    hook = tmp_path / "hook"
    hook.mkdir()
    (hook / "sitecustomize.py").write_text(
        "import os\np = %r\nn = int(open(p).read()) if os.path.exists(p) else 0\nopen(p, 'w').write(str(n + 1))\n"
        "os.environ['HOOK_T'] = 'A' if n == 0 else 't%%d' %% n\nos.environ['HOOK_NEW'] = str(n)\n" % str(hook / "count"))
    stub = tmp_path / "test_fwd_ntt"
    stub.write_text(trace_scripts.STUB)
    stub.chmod(stub.stat().st_mode | stat.S_IEXEC)
    env = dict(os.environ, HOOK_T="A", PYTHONPATH=os.pathsep.join([str(hook)] + [p for p in [os.environ.get("PYTHONPATH")] if p]))
    base, out = tmp_path / "base.json", tmp_path / "trace.jsonl"
    base.write_text(json.dumps(env))
    for _ in range(3):
        subprocess.run([str(stub), "x"], cwd=tmp_path, check=True, timeout=60,
                       env=dict(env, N="8192", HEXL_TRACE_FILE=str(out), HEXL_TRACE_BASE_ENV=str(base), HEXL_TRACE_SCRIPT="s"))
    assert int((hook / "count").read_text()) == 3, "the hook did not run in the stubs"
    got = [json.loads(l) for l in out.read_text().splitlines()]
    assert got == [{"script": "s", "exe": "test_fwd_ntt", "argv": ["x"], "env": {"N": "8192"}}] * 3


def test_committed_build_trace_matches_a_fresh_one_when_both_exist(tmp_path):
    built = HARNESS / "_build" / "script_trace.json"
    if not (os.path.isdir(REF) and built.exists()):
        pytest.skip("needs the reference tree and a built harness")
    sys.path.insert(0, str(HARNESS))
    import trace_scripts
    out = tmp_path / "trace.json"
    assert trace_scripts.trace(REF, out) == 0
    assert json.loads(out.read_text())["invocations"] == json.loads(built.read_text())["invocations"]
