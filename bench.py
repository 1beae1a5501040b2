#!/usr/bin/env python3
"""Flagship benchmark: stub-kubelet pod admission on MI355X.

Measures the BASELINE.json headline: Allocate() latency and
advertised-vs-present GPU correctness at N GPUs requested.  One step = one
pod admission for N GPUs: GetPreferredAllocation(size=N) + Allocate(N ids)
against the live device plugin (real kfd sysfs on a GPU box; synthetic
8*MI355X fake tree elsewhere).

Contract (driver):
  python bench.py --gpus N --steps K --warmup W
prints ONE JSON line from rank 0; multi-rank runs come via torchrun with
one rank per GPU (rank 0 drives the node-local plugin, every rank
participates in the timing barriers).

Such a plain run only sets up, warms up, times the K steps and reports.
--full adds everything else: the per-rank checked matmul, the compiled
C-client latency, and the opt-in --curve / --hbm-probe measurements.
--dump-outputs DIR stores what the last timed step returned, as .npy.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time


def _dist_env():
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    return world, rank, local_rank


def _pin_to_own_l3():
    """Restrict this process to the allowed CPUs that share an L3 cache
    with the CPU it is running on; returns the CPU list (None: not pinned).

    A step is a chain of thread wake-ups between the client, its grpc
    poller and the plugin's server thread.  Left to the scheduler on a
    many-die host those threads share a die in one run and not in the
    next, and identical runs differ by a factor of two (figures in
    docs/benchmarks.md).  The group is the one the scheduler chose for
    this process, so concurrent runs do not all pile onto the same CPUs.
    Must run before any thread is created: only threads started afterwards
    inherit the mask.
    """
    if not hasattr(os, "sched_setaffinity"):
        return None
    try:
        allowed = os.sched_getaffinity(0)
        with open("/proc/self/stat") as f:
            # field 39 (processor); the command name may hold spaces
            here = int(f.read().rsplit(")", 1)[1].split()[36])
        with open(f"/sys/devices/system/cpu/cpu{here}"
                  "/cache/index3/shared_cpu_list") as f:
            shared = set()
            for part in f.read().strip().split(","):
                lo, _, hi = part.partition("-")
                shared.update(range(int(lo), int(hi or lo) + 1))
        cpus = sorted(shared & allowed)
        if not cpus:
            return None
        os.sched_setaffinity(0, cpus)
        return cpus
    except (OSError, ValueError, IndexError):
        return None


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--hbm-probe", action="store_true",
                    help="also run the deep health probe before timing")
    ap.add_argument("--curve", default=None, metavar="N1,N2,...",
                    help="single-process scaling curve: measure each N "
                         "(e.g. 1,2,4,8) back-to-back and report all of "
                         "them in config.curve of the one JSON line")
    ap.add_argument("--sysfs", choices=["auto", "live", "fake"],
                    default="auto",
                    help="topology source: auto = live kfd if present, "
                         "else synthetic 8xMI355X tree; fake forces the "
                         "synthetic tree (full 8-GPU curve on any box)")
    ap.add_argument("--fake-partitions", type=int, default=1,
                    help="with --sysfs fake: CPX-style partitions per GPU "
                         "(8 -> 64 logical devices, BASELINE config 4)")
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline figure does not need: "
                         "per-rank checked GPU matmul, C-client latencies, "
                         "and --curve / --hbm-probe when given")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps write the responses of the "
                         "last step to DIR/<name>.npy")
    ap.add_argument("--cpu-pin", choices=["l3", "none"], default="l3",
                    help="l3: keep the run's threads on the CPUs sharing "
                         "one L3 cache (repeatable timings); none: leave "
                         "placement to the scheduler")
    args = ap.parse_args()
    if (args.curve or args.hbm_probe) and not args.full:
        ap.error("--curve and --hbm-probe are extra measurements: add --full")

    world, rank, local_rank = _dist_env()
    # only rank 0 runs the steps; before torch, which starts threads
    pinned_cpus = None
    if rank == 0 and args.cpu_pin == "l3":
        pinned_cpus = _pin_to_own_l3()

    import torch

    dist = None
    if world > 1:
        import torch.distributed as dist_mod

        dist = dist_mod
        dist.init_process_group(backend="gloo")

    present_gpus = torch.cuda.device_count() if torch.cuda.is_available() else 0
    # a rank only touches a GPU that actually exists (a world size larger
    # than the visible device count happens when the CPU-path bench is
    # launched on a partially-visible box)
    cuda = torch.cuda.is_available() and local_rank < present_gpus

    if cuda:
        torch.cuda.set_device(local_rank)
        # bring the HIP runtime up here, before the harness starts and
        # warms up: left to the first timing barrier it would start its
        # threads between the warmup and the timed steps and disturb them
        torch.cuda.synchronize()
    # ---- advertised-vs-present: every rank touches its own GPU ----
    if cuda and args.full:
        x = torch.ones(1024, 1024, device=f"cuda:{local_rank}")
        y = (x @ x).sum()
        assert float(y) == 1024.0 * 1024 * 1024, "GPU sanity matmul failed"
        torch.cuda.synchronize()

    def barrier_sync():
        if dist is not None:
            dist.barrier()
        if cuda:
            torch.cuda.synchronize()

    probe_summary = None
    if args.hbm_probe and cuda and rank == 0:
        from k8s_device_plugin_amd.native import deep_health_probe

        p = deep_health_probe(device=local_rank, hbm_bytes=1 << 30)
        probe_summary = {
            "healthy": p["healthy"],
            "hbm_gbps": round(p["hbm_gbps"], 1),
            "mfma_tflops": round(p["mfma_tflops"], 1),
        }

    curve_ns = None
    if args.curve:
        curve_ns = sorted({int(x) for x in args.curve.split(",") if x.strip()})

    result = {}
    harness = None
    if rank == 0:
        try:
            harness = _Harness(
                args.gpus if curve_ns is None else 1, sysfs=args.sysfs,
                fake_partitions=args.fake_partitions,
            )
            harness.start()
            if curve_ns is not None:
                # clamp to what the node actually advertises (a live box
                # may expose fewer kfd-visible GPUs than requested)
                curve_ns = [n for n in curve_ns if n <= harness.advertised]
            # warmup
            for _ in range(args.warmup):
                harness.step()
        except Exception as e:
            # fail the whole torchrun job instead of deadlocking peers at
            # the timing barrier
            import traceback

            traceback.print_exc()
            print(f"bench harness failed: {e}", file=sys.stderr, flush=True)
            os._exit(1)

    curve_out = None
    if rank == 0 and curve_ns:
        curve_out = _run_curve(harness, curve_ns, args.steps, args.warmup)

    calls_before = len(harness.alloc_lat_us) if rank == 0 else 0
    barrier_sync()
    t0 = time.perf_counter()
    if rank == 0:
        for _ in range(args.steps):
            harness.step()
    barrier_sync()
    t1 = time.perf_counter()
    elapsed = t1 - t0

    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t[0])

    if rank == 0:
        lat_sorted = sorted(harness.alloc_lat_us)
        alloc_p50_us = statistics.median(lat_sorted)
        alloc_p99_us = lat_sorted[int(len(lat_sorted) * 0.99)]
        pref_p50_us = (
            statistics.median(harness.pref_lat_us) if harness.pref_lat_us else None
        )
        advertised = harness.advertised
        timed_allocates = len(harness.alloc_lat_us) - calls_before
        if args.dump_outputs:
            harness.dump_outputs(args.dump_outputs)
        native_client_p50 = (
            harness.native_client_p50_us() if args.full else None
        )
        harness.stop()

        value = args.gpus * args.steps / elapsed  # device-grants/s, whole job
        out = {
            "metric": "pod_admission_device_grants_per_s",
            "value": round(value, 2),
            "unit": "device-grants/s",
            "n_gpus": args.gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,  # reference publishes no numbers
            "dtype": "n/a",
            "data": "synthetic",
            "config": {
                # BASELINE.json's headline is a compound (Allocate p50 +
                # advertised-vs-present); the scalar `value` is the
                # admission aggregate and the compound's components follow
                "baseline_metric": (
                    "Allocate() p50 latency + advertised-vs-present GPUs "
                    "at 1/2/4/8 MI355X"
                ),
                "model": "stub-kubelet-pod-admission",
                "resource": "amd.com/gpu",
                "devices_per_allocate": args.gpus,
                "parallelism": "node-local",
                "server": harness.server_impl,
                "sysfs": harness.sysfs_kind,
                "advertised_gpus": advertised,
                "present_gpus": present_gpus,
                "pinned_cpus": len(pinned_cpus) if pinned_cpus else 0,
                # Allocate round trips recorded inside the timed window
                "timed_allocates": timed_allocates,
                "allocate_p50_us": round(alloc_p50_us, 1),
                "allocate_p99_us": round(alloc_p99_us, 1),
                "native_client_allocate_p50_us": native_client_p50,
                "native_client_preferred_p50_us": getattr(
                    harness, "native_pref_p50_us", None
                ),
                "preferred_alloc_p50_us": (
                    round(pref_p50_us, 1) if pref_p50_us is not None else None
                ),
                "deep_probe": probe_summary,
                "curve": curve_out,
            },
        }
        print(json.dumps(out), flush=True)

    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    return 0


def _run_curve(harness: "_Harness", ns, steps: int, warmup: int):
    """Measure each N back-to-back in one process: the 1/2/4/8 scaling
    curve of the BASELINE headline (Allocate p50 + advertised-vs-present
    at N GPUs requested), plus hive-packing evidence for the chosen sets."""
    out = []
    for n in ns:
        harness.alloc_lat_us = []
        harness.pref_lat_us = []
        for _ in range(warmup):
            harness.step(n)
        t0 = time.perf_counter()
        for _ in range(steps):
            harness.step(n)
        t1 = time.perf_counter()
        lat = sorted(harness.alloc_lat_us)
        entry = {
            "n": n,
            "admissions_per_s": round(steps / (t1 - t0), 2),
            "device_grants_per_s": round(n * steps / (t1 - t0), 2),
            "ms_per_step": round((t1 - t0) / steps * 1e3, 4),
            "allocate_p50_us": round(statistics.median(lat), 1),
            "allocate_p99_us": round(lat[int(len(lat) * 0.99)], 1),
            "preferred_alloc_p50_us": (
                round(statistics.median(harness.pref_lat_us), 1)
                if harness.pref_lat_us else None
            ),
            "hives_in_chosen_set": harness.hive_count(harness.last_chosen),
        }
        out.append(entry)
    return out


class _Harness:
    """Plugin + stub kubelet over live or synthetic sysfs (rank 0 only)."""

    def __init__(self, n_gpus: int, sysfs: str = "auto",
                 fake_partitions: int = 1):
        self.n = n_gpus
        self.sysfs_mode = sysfs
        self.fake_partitions = fake_partitions
        self.alloc_lat_us = []
        self.pref_lat_us = []
        self.advertised = 0
        self.sysfs_kind = "unknown"
        self.last_chosen = []
        self.last_pref_resp = None
        self.last_alloc_resp = None
        self._tmp = None
        self._mgr = None
        self._kubelet = None
        self._stream_call = None

    def start(self) -> None:
        from k8s_device_plugin_amd.plugin import AMDGPUPlugin, PluginManager
        from k8s_device_plugin_amd.protos import deviceplugin as dp
        from k8s_device_plugin_amd.testing.stub_kubelet import StubKubelet
        from k8s_device_plugin_amd.topology import SysPaths, simple_health_check

        from k8s_device_plugin_amd.testing.sockdir import short_tmp_root

        self._tmp = tempfile.TemporaryDirectory(
            prefix="amdxdp-bench-", dir=short_tmp_root()
        )
        root = self._tmp.name

        live = SysPaths("/")
        use_live = (
            self.sysfs_mode != "fake"
            and os.path.isdir(live.kfd_class)
            and simple_health_check(live)
        )
        if self.sysfs_mode == "live" and not use_live:
            raise RuntimeError("--sysfs live requested but no live kfd found")
        if use_live:
            paths = live
            self.sysfs_kind = "live"
        else:
            from k8s_device_plugin_amd.testing.fakesysfs import build_mi355x_node

            fs = build_mi355x_node(
                os.path.join(root, "fakesys"), n_gpus=max(self.n, 8),
                partitions_per_gpu=self.fake_partitions,
                compute_partition="CPX" if self.fake_partitions > 1 else "SPX",
            )
            paths = fs.paths
            self.sysfs_kind = (
                "fake-8xMI355X" if self.fake_partitions <= 1
                else f"fake-8xMI355X-cpx{self.fake_partitions}"
            )
        self._paths = paths

        dp_dir = os.path.join(root, "device-plugins")
        self._kubelet = StubKubelet(dp_dir).start()
        server_impl = os.environ.get("AMDXDP_SERVER", "native")
        self._mgr = PluginManager(
            lambda res: AMDGPUPlugin(resource=res, paths=paths),
            device_plugin_path=dp_dir,
            server_impl=server_impl,
        )
        self._mgr.run(["gpu"])
        self.server_impl = (
            "native" if self._mgr.plugins["gpu"].native else "python"
        )
        reg = self._kubelet.wait_for_registration()
        self._stub = self._kubelet.connect(reg.endpoint)
        self._dp = dp
        # on a 1-GPU node there are no GPU-GPU links, so the plugin degrades
        # to kubelet-default allocation (no GetPreferredAllocation) exactly
        # like the reference (plugin.go:86-89,210-217)
        self.preferred_available = reg.options.get_preferred_allocation_available

        # initial ListAndWatch: the advertised device set
        call = self._stub.ListAndWatch(dp.Empty())
        first = next(iter(call))
        self._stream_call = call
        # only Healthy (kfd-backed) devices are schedulable; cgroup-masked
        # peer GPUs are advertised Unhealthy on restricted boxes
        self.device_ids = sorted(
            d.ID for d in first.devices if d.health == "Healthy"
        )
        self.advertised = len(self.device_ids)
        if self.advertised < self.n:
            raise RuntimeError(
                f"advertised {self.advertised} healthy devices < requested {self.n}"
            )

    def step(self, n: int = None) -> None:
        dp = self._dp
        if n is None:
            n = self.n
        # 1. GetPreferredAllocation for N devices (when advertised)
        if self.preferred_available:
            req = dp.PreferredAllocationRequest()
            cr = req.container_requests.add()
            cr.available_deviceIDs.extend(self.device_ids)
            cr.allocation_size = n
            t0 = time.perf_counter()
            resp = self._stub.GetPreferredAllocation(req, timeout=10)
            t1 = time.perf_counter()
            self.pref_lat_us.append((t1 - t0) * 1e6)
            self.last_pref_resp = resp
            chosen = list(resp.container_responses[0].deviceIDs)
        else:
            chosen = self.device_ids[:n]
        self.last_chosen = chosen

        # 2. Allocate them
        areq = dp.AllocateRequest()
        areq.container_requests.add().devices_ids.extend(chosen)
        t0 = time.perf_counter()
        aresp = self._stub.Allocate(areq, timeout=10)
        t1 = time.perf_counter()
        self.alloc_lat_us.append((t1 - t0) * 1e6)
        self.last_alloc_resp = aresp
        specs = aresp.container_responses[0].devices
        assert len(specs) == 1 + 2 * n, (
            f"expected /dev/kfd + 2 nodes per device, got {len(specs)}"
        )

    def dump_outputs(self, out_dir: str) -> None:
        """Write what the last step() received as <out_dir>/<name>.npy.

        The step's results are protobuf messages.  Their fields are stored
        decoded -- granted_device_indices (positions of the granted devices
        in the sorted advertised ID list), allocate_device_nodes (one row
        per DeviceSpec: kind 0 /dev/kfd, 1 card, 2 renderD, 3 other; the
        node number; 1 if host and container path agree) and
        allocate_counts (devices, mounts, envs, annotations, CDI devices)
        -- and, for an exact comparison, as their deterministic wire
        encoding, one byte per float32 element (a few hundred bytes).  The
        requests are a pure function of the advertised list and of --gpus,
        so two builds run with the same arguments on the same node can be
        compared array for array.
        """
        import re

        import numpy as np

        if self.last_alloc_resp is None:
            raise RuntimeError("--dump-outputs needs at least one step")

        def wire(msg):
            raw = msg.SerializeToString(deterministic=True)
            return np.frombuffer(raw, dtype=np.uint8).astype(np.float32)

        def save(name, arr):
            np.save(os.path.join(out_dir, name + ".npy"), arr)

        os.makedirs(out_dir, exist_ok=True)
        index = {d: i for i, d in enumerate(self.device_ids)}
        save("granted_device_indices",
             np.array([index[d] for d in self.last_chosen], dtype=np.float64))

        cr = self.last_alloc_resp.container_responses[0]
        nodes = []
        for spec in cr.devices:
            m = re.fullmatch(r"/dev/(?:kfd|dri/(card|renderD)(\d+))",
                             spec.host_path)
            if m is None:
                kind, num = 3, -1
            elif m.group(1) is None:
                kind, num = 0, -1
            else:
                kind, num = (1 if m.group(1) == "card" else 2), int(m.group(2))
            nodes.append(
                [kind, num, float(spec.host_path == spec.container_path)]
            )
        save("allocate_device_nodes",
             np.array(nodes, dtype=np.float64).reshape(-1, 3))
        save("allocate_counts", np.array(
            [len(cr.devices), len(cr.mounts), len(cr.envs),
             len(cr.annotations), len(cr.cdi_devices)], dtype=np.float64))

        save("allocate_response_bytes", wire(self.last_alloc_resp))
        if self.last_pref_resp is not None:
            save("preferred_response_bytes", wire(self.last_pref_resp))

    def hive_count(self, device_ids) -> int:
        """Distinct xGMI hives spanned by a device-ID set (1 = packed)."""
        try:
            from k8s_device_plugin_amd.topology import (
                KFDTopology, discover_gpus,
            )

            topo = KFDTopology.load(self._paths)
            devs = discover_gpus(self._paths, topology=topo, strict=False)
            hives = set()
            for did in device_ids:
                d = devs.get(did)
                if d is None or d.node_id not in topo.nodes:
                    return -1
                hives.add(topo.nodes[d.node_id].hive_id)
            return len(hives)
        except Exception:
            return -1

    def native_client_p50_us(self):
        """Allocate p50 measured with the C/nghttp2 bench client — the
        latency a compiled kubelet sees, without Python-client overhead."""
        import subprocess

        exe = os.path.join(
            os.path.dirname(os.path.abspath(__file__)),
            "k8s_device_plugin_amd", "native", "benchclient",
        )
        src = exe + ".cpp"
        if not os.path.exists(exe) and os.path.exists(src):
            try:
                subprocess.run(
                    ["g++", "-O2", "-std=c++17", src, "-o", exe, "-ldl"],
                    check=True, capture_output=True, timeout=120,
                )
            except Exception:
                return None
        if not os.path.exists(exe) or not getattr(self, "server_impl", "") == "native":
            return None
        sock = self._mgr.plugins["gpu"].socket_path
        try:
            out = subprocess.run(
                [exe, sock, self.device_ids[0], "2000",
                 ",".join(self.device_ids), str(self.n)],
                capture_output=True, text=True, timeout=120,
            )
            if out.returncode != 0:
                return None
            rec = json.loads(out.stdout.strip().splitlines()[-1])
            self.native_pref_p50_us = rec.get("preferred_p50_us")
            return rec["allocate_p50_us"]
        except Exception:
            return None

    def stop(self) -> None:
        if self._stream_call is not None:
            self._stream_call.cancel()
        if self._mgr is not None:
            self._mgr.stop()
        if self._kubelet is not None:
            self._kubelet.stop()
        if self._tmp is not None:
            self._tmp.cleanup()


if __name__ == "__main__":
    sys.exit(main())
