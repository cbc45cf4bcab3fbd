"""Times the device-buffer form of the trace commitment for an arbitrary configuration (bring-up / tuning aid).
    python scripts/time_config.py <field 1|2> <ext> <log2 R> <log2 blowup> <n_cols> <n_traces> [hasher id] [--hasher NAME|id]
(hasher: 0 / blake3 = BLAKE3, 1 / sha3 = Sha3_256, 16 / rp64 = Rp64_256, 18 / rpjive = RpJive64_256, 20 / griffin = GriffinJive64_256; the profile marks split the time into the
transform, "hash_rows" and "merkle")"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import starkpack_winterfell_amd.capi as capi

HASHERS = {"blake3": capi.BLAKE3, "sha3": capi.SHA3_256, "rp64": capi.RP64_256, "rpjive": capi.RPJIVE64_256, "griffin": capi.GRIFFINJIVE64_256}
argv = sys.argv[1:]
hasher = capi.BLAKE3
if "--hasher" in argv:
    at = argv.index("--hasher")
    name = argv[at + 1].lower()
    hasher = HASHERS[name] if name in HASHERS else int(name)
    del argv[at:at + 2]
elif len(argv) > 6:
    hasher = int(argv[6])
field, ext, logR, logB, n_cols, n_traces = (int(x) for x in argv[:6])
dev = torch.device("cuda", 0)
ctx = capi.Context(0)
w = 1 if field == 1 else 2
R, N = 1 << logR, 1 << (logR + logB)
gen = torch.Generator(device=dev); gen.manual_seed(1)
trace = torch.randint(0, 2**62, (n_traces * n_cols * R * ext * w,), dtype=torch.int64, device=dev, generator=gen)
polys = torch.empty_like(trace)
rw = 8 * ((n_cols * ext + 7) // 8)
lde = torch.empty(n_traces * N * rw * w, dtype=torch.int64, device=dev)
leaves = torch.empty((N, 32), dtype=torch.uint8, device=dev)
nodes = torch.empty((N, 32), dtype=torch.uint8, device=dev)
p = capi.make_params(field, ext, logR, logB, n_cols, n_traces, hasher=hasher)
s = torch.cuda.Stream(device=dev)
ctx.profile_enable(2)
with torch.cuda.stream(s):
    for _ in range(2):
        ctx.trace_commit_dev(p, trace.data_ptr(), polys.data_ptr(), lde.data_ptr(), leaves.data_ptr(), nodes.data_ptr(), s.cuda_stream)
    torch.cuda.synchronize(); ctx.profile_read()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    K = 5
    e0.record()
    for _ in range(K):
        ctx.trace_commit_dev(p, trace.data_ptr(), polys.data_ptr(), lde.data_ptr(), leaves.data_ptr(), nodes.data_ptr(), s.cuda_stream)
    e1.record(); torch.cuda.synchronize()
acc = {}
for k, v in ctx.profile_read():
    acc.setdefault(k, []).append(v)
print(f"field={field} ext={ext} R=2^{logR} blowup={1<<logB} cols={n_cols} traces={n_traces} hasher={hasher}: {e0.elapsed_time(e1)/K:.3f} ms",
      {k: round(sum(v)/len(v), 4) for k, v in acc.items()})
