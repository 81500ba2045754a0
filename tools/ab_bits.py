"""Are two builds of the library bit-identical on a parity case?  (GPU box)
    python tools/ab_bits.py dump out.npz [case] [key=value ...]   # with GT_HIP_LIB selecting the build
    python tools/ab_bits.py cmp a.npz b.npz
`case` is a name from cases.CASES or cases.ORACLE_ONLY_CASES (default acoustic_mlp); every key=value is an engine option handed to
run_hip_case(engine_options=...), e.g. fused_dstack=2 split_first_layer=0; comm=1 is no engine option: it attaches a one-rank communicator
(run_hip_case(comm_world_1=True)) and switches its collectives on.  One dump per process."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

if sys.argv[1] == "dump":
    import cases as C
    from hip_runner import run_hip_case
    rest = sys.argv[3:]
    name = rest.pop(0) if rest and "=" not in rest[0] else "acoustic_mlp"
    case = C.CASES[name] if name in C.CASES else C.ORACLE_ONLY_CASES[name]
    options = {k: int(v) for k, v in (kv.split("=", 1) for kv in rest)}
    comm = bool(options.pop("comm", 0))
    if comm:      # a one-rank communicator whose collectives are issued: the data-parallel schedule
        options.setdefault("comm_force", 1)
    got = run_hip_case(case, engine_options=options or None, comm_world_1=comm)
    np.savez(sys.argv[2], **{k: np.asarray(v) for k, v in got.items()})
else:
    a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
    bad = sorted(set(a.files) ^ set(b.files))
    bad += [k for k in a.files if k in b.files and not np.array_equal(a[k].view(np.uint8) if a[k].dtype.kind == "f" else a[k], b[k].view(np.uint8) if b[k].dtype.kind == "f" else b[k])]
    print("%d arrays, %d differ%s" % (len(a.files), len(bad), (": " + " ".join(bad[:8])) if bad else ""))
    sys.exit(1 if bad else 0)
