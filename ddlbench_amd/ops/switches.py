"""The DDLB_* backend switches: one table and the only code in ops/ and
models/ that reads the environment.

A switch names an environment variable, the values it takes and its
default. ``resolve`` answers which value holds now: an explicit argument
wins, otherwise the environment is read at the time of the call, and
anything outside the allowed values is a ValueError. Flipping a default is
a one-word change in ``SWITCHES``; docs/ENV.md lists the same rows."""

from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Optional, Tuple


@dataclass(frozen=True)
class Switch:
    env: str
    values: Tuple[str, ...]
    default: str


SWITCHES = {
    "join": Switch("DDLB_JOIN", ("1", "0"), "1"),
    "gate": Switch("DDLB_GATE", ("1", "0"), "1"),
    "maxpool": Switch("DDLB_MAXPOOL", ("1", "0"), "1"),
    "conv_tail": Switch("DDLB_CONV_TAIL", ("native", "eager"), "native"),
    "stem": Switch("DDLB_STEM", ("native", "library"), "library"),
    "grouped": Switch("DDLB_GROUPED", ("native", "library"), "library"),
    "lstm": Switch("DDLB_LSTM", ("auto", "native", "library"), "auto"),
    "attn_score": Switch("DDLB_ATTN_SCORE", ("auto", "native", "torch"),
                         "auto"),
    "attn_ctx": Switch("DDLB_ATTN_CTX", ("library", "native", "torch"),
                       "library"),
}


def check(what: str, value, allowed) -> str:
    """``value`` if it is one of ``allowed``, else the ValueError every
    backend choice raises."""
    if value not in allowed:
        names = ", ".join(allowed[:-1]) + " or " + allowed[-1]
        raise ValueError(f"{what} backend must be {names}, got {value!r}")
    return value


def resolve(name: str, explicit: Optional[str] = None) -> str:
    """The value of switch ``name``: ``explicit`` if given, else its
    environment variable as it is now, else its default."""
    sw = SWITCHES[name]
    value = os.environ.get(sw.env, sw.default) if explicit is None \
        else explicit
    return check(sw.env, value, sw.values)


def enabled(name: str) -> bool:
    """A "1"/"0" switch as a bool."""
    return resolve(name) == "1"
