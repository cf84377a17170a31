"""Child process of tests/test_refine_gpu.py: a ONE-rank `nccl` (= RCCL) process group on cuda:0 with
LIST_FORCE_COLLECTIVES=1, so that the coarse-to-fine grid's sharded passes (lattice and refined list, split with
parallel.shard_range and all-gathered with parallel.gather_ragged_points) run through real collectives.  Prints one
JSON line: whether the sharded refined volume equals the unsharded one bit for bit."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
os.environ.setdefault("MASTER_PORT", str(29900 + os.getpid() % 500))
os.environ["LIST_FORCE_COLLECTIVES"] = "1"
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
from oracle import fill, synth  # noqa: E402
from list_amd import arguments, utils  # noqa: E402
from list_amd.train import _Module  # noqa: E402

cfg = arguments.default_config(vox_res=32, train_batch_size=1, mcube_znum=48, test_pointnum=5000)
cfg.device = dev
net = fill.fill_state(utils.get_class("network.models.LIST")(cfg), seed=2).eval().to(dev)
ex = utils.get_class("network.executors.LIST")(cfg, _Module(net))
img = torch.from_numpy(synth.uniform(78, (1, 3, 64, 64))).to(dev)
with torch.no_grad():
    enc = net.encode(img)
net.encode = lambda *a, **k: enc                   # MIOpen is not run-to-run deterministic: one set of maps
dense = ex.predict_grid(img, shard=False)[0]
level = float(dense.median())
a = ex.predict_grid(img, shard=False, refine=4, level=level)[0]
stats_a = dict(ex.last_grid_stats)
b = ex.predict_grid(img, shard=True, refine=4, level=level)[0]
torch.cuda.synchronize()
print(json.dumps({"backend": dist.get_backend(), "world": dist.get_world_size(), "equal": bool(torch.equal(a, b)),
                  "stats_equal": stats_a == ex.last_grid_stats, "refined": stats_a["refined"]}))
dist.destroy_process_group()
