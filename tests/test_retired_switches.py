"""Switches whose kernels were removed must fail loudly, not be ignored."""

import pytest

from mapreduce_amd import ops


def test_retired_switch_raises_and_names_the_variable():
    for name in ops.RETIRED_SWITCHES:
        with pytest.raises(RuntimeError) as ei:
            ops.check_retired_switches({name: "1", "MR_TOK_GPOS": "0"})
        assert name in str(ei.value)
        assert "removed" in str(ei.value)
    # set to anything, "0" included: the variable no longer means anything
    with pytest.raises(RuntimeError, match="MR_TOK_BSPILL"):
        ops.check_retired_switches({"MR_TOK_BSPILL": "0"})


def test_clean_environment_passes(monkeypatch):
    for name in ops.RETIRED_SWITCHES:
        monkeypatch.delenv(name, raising=False)
    ops.check_retired_switches()  # os.environ
    # the switches that remain are not retired
    ops.check_retired_switches({"MR_TOKENIZE_V6": "1", "MR_TOK_GPOS": "0",
                                "MR_RADIX_V2": "1"})


def test_entry_points_check_the_environment(monkeypatch):
    """require_gpu_ext() checks on every call, ops.ext() on the first call
    of a process, whether or not the extension is built or a GPU is there."""
    monkeypatch.setenv("MR_TOKENIZE_V5", "1")
    with pytest.raises(RuntimeError, match="MR_TOKENIZE_V5"):
        ops.require_gpu_ext()
    monkeypatch.setattr(ops, "_switches_checked", False)
    with pytest.raises(RuntimeError, match="MR_TOKENIZE_V5"):
        ops.ext()
