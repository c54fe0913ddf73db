"""Cost of per-point parameter fields: VonMises3D on the headline mix (benchlib.workloads "von_mises_mixed"; the
plastic share of the timed launch is printed) through ResidentState's Newton-iteration launch -- sparse history, packed plastic strain, every tangent row --
with 0, 1 (p_y0) and 5 parameter fields.  Kernel time from the HIP events of the context option "timing" (the kernels alone),
median of the timed iterations, next to the algorithmic bytes: the 0-field launch's plus 8 B per point per field.  The state's
arrays are placed as one interleaved VMM working set (placement="vmm", DESIGN.md 6: reproducible to ~2 %; torch's own allocations
spread over 10-28 %), and the configurations run `rounds` times in turn, each with fresh arrays.

    python tools/field_bench.py [n=1e8] [iterations=10] [rounds=2]
One JSON line per configuration and round."""

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import fenics_constitutive_amd as fc  # noqa: E402
from benchlib.workloads import VM_P, synth_inputs  # noqa: E402
from fenics_constitutive_amd.device import read_counters  # noqa: E402
from fenics_constitutive_amd.resident import ResidentState  # noqa: E402

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 10
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 2
dev = torch.device("cuda", 0)
os.environ.setdefault("FCAMD_SMALL_CALL_WARNING", "0")

for rnd, nf in [(r, nf) for r in range(rounds) for nf in (0, 1, 5)]:
    names = ("p_y0", "p_ka", "p_mu", "p_y00", "p_w")[:nf]
    law = fc.VonMises3D({k: (np.full(n, v) if k in names else v) for k, v in VM_P.items()})
    grad, stress0, hist0 = synth_inputs("von_mises_3d", "loguniform", n, 7, dev)
    g = grad()
    st = ResidentState(law, n, device=dev, stress0=stress0, history0=hist0, placement="vmm")
    del stress0, hist0
    st.evaluate(0.0, 1.0, g)
    m = law._handle(0)
    m.ctx.set_option("timing", 1)
    ms = []
    for _ in range(iters + 2):
        st._launch(0.0, 1.0, g, st.tangent, sparse_tangent=False)
        ms.append(m.last_kernel_ms())
    m.ctx.set_option("timing", 0)
    stats = read_counters(st._counters)  # (the state's own counters: the last launch)
    ms = sorted(ms[2:])
    plastic = stats.n_plastic / n
    # algorithmic bytes of the 0-field launch: 464 B/pt elastic, 568 plastic (benchlib.workloads: von_mises_mixed; sparse history, the
    # whole tangent), + 8 per field
    bytes_pt = 464 + (568 - 464) * plastic + 8 * nf
    print(json.dumps({"round": rnd, "fields": nf, "names": list(names), "n": n, "ms_median": round(ms[len(ms) // 2], 4), "ms_min": round(ms[0], 4),
                      "plastic_fraction": round(plastic, 4), "algorithmic_bytes_per_point": round(bytes_pt, 1),
                      "TB_s": round(bytes_pt * n / (ms[len(ms) // 2] * 1e-3) / 1e12, 3)}), flush=True)
    del st, law, g, grad
    torch.cuda.empty_cache()
