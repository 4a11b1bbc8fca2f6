"""The environment knobs are listed three times by hand: where the library reads them (env_reload), where the Python wrapper
watches them for a change (ops._ENV_KNOBS) and where they are documented (KNOBS.md).  A knob missing from ops._ENV_KNOBS is
silently never re-read, so the three lists are held together here."""
import os
import re

from longterm360fov_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "longterm360fov_amd", "csrc")
READ = re.compile(r"\b(?:getenv|env_flag)\s*\(\s*\"(FOV_[A-Z0-9_]+)\"\s*\)")        # env_flag: env_reload's "equals 1" reader
GETENV_CALL = re.compile(r"\bgetenv\s*\(")


def sources():
    return {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h"))}


def test_the_knobs_read_are_the_knobs_watched_and_documented():
    src = sources()
    read = {name for text in src.values() for name in READ.findall(text)}
    assert len(read) >= 27 and "FOV_NO_WIDE16" in read and "FOV_TWO_LAUNCHES" in read
    assert len(set(ops._ENV_KNOBS)) == len(ops._ENV_KNOBS)
    assert read == set(ops._ENV_KNOBS), sorted(read ^ set(ops._ENV_KNOBS))
    doc = open(os.path.join(ROOT, "KNOBS.md")).read()
    assert [n for n in sorted(read) if not re.search(r"\b%s\b" % n, doc)] == []


def test_only_env_reload_reads_the_environment():
    """Nothing on a launch path calls getenv: the one source that does holds env_reload."""
    calling = [f for f, text in sources().items() if GETENV_CALL.search(text)]
    assert len(calling) == 1 and "void env_reload()" in sources()[calling[0]], calling
