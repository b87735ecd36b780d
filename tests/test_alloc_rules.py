"""Source rule of the library's device allocations (CPU only).  WA_DEV_POISON=1 fills every device block before it is handed out
(csrc/weldacs.hip: poison_fill; tests/test_gpu_poisoned_scratch.py runs the planning calls that way).  That holds only while every
allocation goes through the two places that fill: dev_malloc (and with it dalloc / DevBuf) and the context's allocator, which takes its
whole blocks from dev_malloc and its chunks from arena_chunk.  Both stand between marker lines in weldacs.hip; a later file that calls
the runtime's allocators itself would step around the poison.

WA_DEV_GUARD=1 puts every dev_malloc block between two red zones and checks them when the block is given back (dev_free,
tests/test_gpu_red_zones.py).  That holds only while every block goes back through dev_free: hipFree, too, may be called between the
marker lines only, and the host files call dev_free wherever they called hipFree before the zones existed."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "welding_robot_amd", "csrc")
BEGIN, END = "// ---- device allocation: begin", "// ---- device allocation: end"
ALLOCATORS = r"\bhipMalloc\w*\(|\bhipExtMallocWithFlags\(|\bhipMemCreate\(|\bhipFree\("
HIPFREE_CALLS_BEFORE = 48     # hipFree( outside the marker lines in the commit before dev_free existed (comments not counted)


def test_device_memory_is_allocated_between_the_marker_lines_only():
    files = sorted(f for ext in ("*.inc", "*.hip", "*.hpp", "*.h") for f in glob.glob(os.path.join(CSRC, ext)))
    assert len(files) > 40
    inside_hits, bad, regions = 0, [], 0
    for f in files:
        inside = False
        for n, line in enumerate(open(f), 1):
            if line.startswith(BEGIN):
                assert not inside and f.endswith("weldacs.hip"), (f, n)
                inside, regions = True, regions + 1
            elif line.startswith(END):
                assert inside, (f, n)
                inside = False
            elif re.search(ALLOCATORS, line.split("//")[0]):
                if inside:
                    inside_hits += 1
                else:
                    bad.append("%s:%d %s" % (os.path.basename(f), n, line.strip()))
        assert not inside, f
    assert not bad, "\n".join(bad)
    assert regions == 2 and inside_hits >= 6      # dev_malloc's two calls and arena_chunk's, hipFree in dev_malloc and dev_free: the rule still looks at something


def test_device_memory_is_given_back_through_dev_free():
    """outside the marker lines csrc calls dev_free at least as often as it called hipFree before (its declaration is not a call)"""
    calls = 0
    for f in sorted(f for ext in ("*.inc", "*.hip", "*.hpp", "*.h") for f in glob.glob(os.path.join(CSRC, ext))):
        inside = False
        for line in open(f):
            if line.startswith(BEGIN) or line.startswith(END):
                inside = line.startswith(BEGIN)
            elif not inside and not line.startswith("static hipError_t dev_free("):
                calls += len(re.findall(r"\bdev_free\(", line.split("//")[0]))
    assert calls >= HIPFREE_CALLS_BEFORE, calls


def test_the_marked_regions_hold_the_fill():
    """the hipMalloc region is dev_malloc with its poison_fill; the context allocator fills what it hands out itself"""
    src = open(os.path.join(CSRC, "weldacs.hip")).read()
    region = src.split(BEGIN)[1].split(END)[0]
    assert "static hipError_t dev_malloc(" in region and "poison_fill(" in region and "g_alloc_ctx" in region
    # ... and dev_free with its zone comparison: both zones copied to the host, every byte held against the guard byte
    assert "static hipError_t dev_free(" in region and "guard_arm(" in region and "zone comparison" in region
    assert region.count("hipMemcpyDeviceToHost") >= 2 and "!= gb" in region and "g_guard_table" in region
    assert src.count("poison_fill(c, *out, bytes, false)") >= 2      # ctx_alloc_bytes: the arena's blocks and the whole ones
