"""The native sources as text, for the tests that assert something of an entry's definition (a function-try-block closed by
LINNA_CATCH_INT / LINNA_CATCH_SIZE) wherever the entry lives: a subsystem's file holds its kernels, its launch code and
its C entries, so an entry's home is not one file."""
import glob
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hip_sources():
    """The concatenated text of every linna_amd/csrc/*.hip, in name order."""
    return "".join(open(p).read() for p in sorted(glob.glob(os.path.join(ROOT, "linna_amd", "csrc", "*.hip"))))
