"""Record tests/pins/rollout_sha256.json: python scratch/gen_rollout_pins.py COMMIT [out.json]   (needs the GPU)

Run it with the library built from the commit whose rollouts are to be pinned and pass that commit's id; the file says which commit
its hashes came from.  Every case runs in two fresh engines: a case whose two digests differ is not reproducible, is left out of the
file, is named with what differed and makes the exit status 1 (tests/test_gpu_rollout_pins.py then fails its coverage test).
tests/test_gpu_rollout_pins.py asserts the hashes."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "train-procgen-pytorch_amd"), os.path.join(ROOT, "tests")]
from rollout_pin_cases import CASES, PIN_FILE, run_case

commit = sys.argv[1]
out = sys.argv[2] if len(sys.argv) > 2 else PIN_FILE
pins, unstable = {}, []
for name in CASES:
    t0 = time.time()
    a, b = run_case(name), run_case(name)
    diff = sorted(k for k in a if a[k] != b[k])
    print(name, f"{(time.time() - t0) / 2:.2f} s per run", "UNSTABLE: " + ", ".join(diff) if diff else {k: v[:12] for k, v in a.items()}, flush=True)
    if diff:
        unstable.append(name)
    else:
        pins[name] = a
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    json.dump({"commit": commit, "what": "sha256 of the float32 bytes of what each rollout of tests/rollout_pin_cases.py leaves behind", "sha256": pins},
              f, indent=1, sort_keys=True)
    f.write("\n")
print("wrote", out, "-- unstable cases left out:", unstable)
sys.exit(1 if unstable else 0)
