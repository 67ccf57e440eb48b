"""Record tests/pins/resblock_bf16_sha256.json: python scratch/gen_resblock_pins.py COMMIT [out.json]   (needs the GPU)

Run it with the library built from the commit whose outputs are to be pinned and pass that commit's id; the file says which
commit its hashes came from.  tests/test_gpu_resblock_pins.py asserts them."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "train-procgen-pytorch_amd"), os.path.join(ROOT, "tests")]
from resblock_pin_cases import CASES, PIN_FILE, case_id, run_case
from mi355.engine import Engine

commit = sys.argv[1]
out = sys.argv[2] if len(sys.argv) > 2 else PIN_FILE
eng = Engine("impala", n_steps=4, n_envs=4, n_actions=15, max_batch=16, precision="bf16")
pins = {}
for c in CASES:
    pins[case_id(*c)] = run_case(eng, *c)
    print(case_id(*c), {k: v[:12] for k, v in pins[case_id(*c)].items()}, flush=True)
eng.close()
with open(out, "w") as f:
    json.dump({"commit": commit, "what": "sha256 of the float32 bytes of every output of Engine.op_resblock, bf16 precision", "sha256": pins}, f, indent=1, sort_keys=True)
    f.write("\n")
print("wrote", out)
