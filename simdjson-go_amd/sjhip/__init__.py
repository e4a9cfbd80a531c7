"""sjhip -- Python mirror of the simdjson-go backend API on top of libsjhip (MI355X / gfx950).

Mirrors the reference's backend symbol set (simdjson_other.go:29-76):
    SupportedCPU() -> supported()          Parse(b, reuse, opts...) -> parse(...)
    ParseND(b, reuse, opts...) -> parse_nd(...)    WithCopyStrings(bool) -> copy_strings=...
    ParseNDStream(r, res, reuse) -> parse_nd_stream(reader, ...)   (a generator instead of a channel)
"""
from ._lib import SjhipMissing, lib  # noqa: F401
from .api import (TYPE_ARRAY, TYPE_BOOL, TYPE_FLOAT, TYPE_INT, TYPE_NULL, TYPE_OBJECT, TYPE_STRING, TYPE_UINT, Aggregate, Context, Groups,  # noqa: F401
                  MultiContext, Order, ParsedJson, ParseError, Schema, parse, parse_nd, stage1, supported)
from .stream import cut_blocks, parse_nd_stream  # noqa: F401
