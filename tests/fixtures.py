"""Fixture loading for tests / bench: tests/data/<name>.json.xz (see tools/make_fixtures.py)."""
import contextlib
import functools
import lzma
import os

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")

ALL = ["apache_builds", "canada", "citm_catalog", "github_events", "gsoc-2018", "instruments", "marine_ik",
       "mesh", "mesh.pretty", "numbers", "parking-citations", "payload-large", "payload-medium",
       "payload-small", "random", "twitter", "twitterescaped", "update-center"]


@functools.lru_cache(maxsize=None)
def load(name: str) -> bytes:
    with open(os.path.join(DATA, name + ".json.xz"), "rb") as f:
        return lzma.decompress(f.read())


@contextlib.contextmanager
def nd_shard_limits(limit_bytes, shard_bytes):
    """An ND message of more than limit_bytes (and more than 1 MiB) parsed inside the block is cut into shards of about
    shard_bytes (SJHIP_ND_LIMIT_BYTES / SJHIP_ND_SHARD_BYTES, parse_api.hip): the sharded path on documents of a few megabytes.
    The variables are read by the parse call, so the parse belongs inside the block; the result stays sharded after it."""
    os.environ["SJHIP_ND_LIMIT_BYTES"] = str(limit_bytes)
    os.environ["SJHIP_ND_SHARD_BYTES"] = str(shard_bytes)
    try:
        yield
    finally:
        del os.environ["SJHIP_ND_LIMIT_BYTES"], os.environ["SJHIP_ND_SHARD_BYTES"]
