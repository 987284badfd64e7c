"""ops.switches is the one table of DDLB_* backend switches and the one
reader of the environment in ops/ and models/; docs/ENV.md lists the same
rows. No device needed."""

import pathlib
import re

import pytest
import torch

from ddlbench_amd import ops
from ddlbench_amd.ops.switches import SWITCHES, enabled, resolve

_ROOT = pathlib.Path(__file__).resolve().parent.parent
_NAMES = ("join", "gate", "maxpool", "conv_tail", "stem", "grouped", "lstm",
          "attn_score", "attn_ctx")


def test_the_table_has_exactly_the_known_rows():
    assert tuple(SWITCHES) == _NAMES
    envs = [sw.env for sw in SWITCHES.values()]
    assert len(set(envs)) == len(envs)
    for sw in SWITCHES.values():
        assert sw.env.startswith("DDLB_") and sw.default in sw.values
        with pytest.raises(AttributeError):
            sw.default = "other"        # a frozen record


@pytest.mark.parametrize("name", _NAMES)
def test_resolve(name, monkeypatch):
    sw = SWITCHES[name]
    other = next(v for v in sw.values if v != sw.default)
    monkeypatch.delenv(sw.env, raising=False)
    assert resolve(name) == sw.default
    monkeypatch.setenv(sw.env, other)           # read at the time of the call
    assert resolve(name) == other
    assert resolve(name, sw.default) == sw.default      # explicit wins
    monkeypatch.setenv(sw.env, "fastest")
    with pytest.raises(ValueError) as e:
        resolve(name)
    for word in (sw.env, "backend", "'fastest'") + sw.values:
        assert word in str(e.value)
    assert resolve(name, other) == other    # explicit: environment not read
    monkeypatch.delenv(sw.env)
    with pytest.raises(ValueError, match="'nearly'"):
        resolve(name, "nearly")


@pytest.mark.parametrize("name", ["join", "gate", "maxpool"])
def test_enabled(name, monkeypatch):
    env = SWITCHES[name].env
    monkeypatch.delenv(env, raising=False)
    assert enabled(name) is True
    monkeypatch.setenv(env, "0")
    assert enabled(name) is False
    monkeypatch.setenv(env, "off")              # neither "1" nor "0"
    with pytest.raises(ValueError, match=env):
        enabled(name)


def test_callers_see_the_switches(monkeypatch):
    from ddlbench_amd.ops import conv, functional
    monkeypatch.setenv("DDLB_JOIN", "0")
    monkeypatch.setenv("DDLB_GATE", "0")
    assert not conv.join_enabled() and not functional.gate_enabled()
    monkeypatch.setenv("DDLB_MAXPOOL", "yes")
    with pytest.raises(ValueError, match="DDLB_MAXPOOL"):
        conv.convert_convs(torch.nn.Sequential(torch.nn.MaxPool2d(2)))


def test_no_other_reader_of_the_environment():
    pkg = _ROOT / "ddlbench_amd"
    files = sorted((pkg / "ops").glob("*.py")) \
        + sorted((pkg / "models").glob("*.py"))
    assert pkg / "ops" / "switches.py" in files and len(files) > 5
    for path in files:
        if path.name == "switches.py":
            continue
        text = path.read_text()
        assert "os.environ" not in text and "getenv" not in text, path


def test_env_md_lists_every_row():
    text = (_ROOT / "docs" / "ENV.md").read_text()
    assert "DDLB_WGRAD" not in text
    for sw in SWITCHES.values():
        rows = re.findall(rf"^\| `{sw.env}` \|(.*?)\|(.*?)\|", text, re.M)
        assert len(rows) == 1, sw.env
        values, default = rows[0]
        assert values.strip() == ", ".join(f"`{v}`" for v in sw.values)
        assert default.strip() == f"`{sw.default}`"


@pytest.mark.parametrize("backend", ["nativ", "library", "", None])
def test_unknown_kernel_backend_is_an_error(backend):
    with pytest.raises(ValueError, match="backend"):
        ops.use_native(torch.device("cpu"), backend)
    from ddlbench_amd.ops import modules
    with pytest.raises(ValueError, match="backend"):
        modules.set_default_backend(backend)
    assert modules.default_backend() == "auto"


def test_known_kernel_backends_on_cpu():
    assert ops.use_native(torch.device("cpu"), "auto") is False
    assert ops.use_native(torch.zeros(1), "torch") is False
