"""bench.py's training window with loss_scale="dynamic" (DESIGN section 6): the benchmark itself, unchanged, with the
trainer's default switched.  Same arguments as bench.py; compare with `bench.py --dtype f16` on the same box."""
import os, runpy, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from ir2rgb_amd import vid2vid as V
V.DEFAULTS["loss_scale"] = "dynamic"
sys.argv[0] = os.path.join(ROOT, "bench.py")
runpy.run_path(sys.argv[0], run_name="__main__")
