"""GPU tests: run on a real MI355X box (pytest -m gpu).

Covers BASELINE.json config 2 (live kfd enumeration + Allocate paths), the
raw-ioctl shim against real /dev/dri nodes, and the gfx950 deep health
probe (MFMA/LDS/HBM on-device verification).
"""

import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _require_gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")


@pytest.fixture(scope="module")
def live_devices():
    _require_gpu()
    from k8s_device_plugin_amd.topology import SysPaths, discover_gpus

    paths = SysPaths("/")
    devs = discover_gpus(paths)
    assert devs, "no AMD GPUs discovered on a GPU box"
    return paths, devs


def test_live_kfd_discovery(live_devices):
    from k8s_device_plugin_amd.topology import KFDTopology

    paths, devs = live_devices
    topo = KFDTopology.load(paths)
    gpu_nodes = topo.gpu_nodes()
    assert len(gpu_nodes) >= 1
    for node in gpu_nodes:
        assert node.properties.get("gfx_target_version", 0) >= 90000
        # MI355X: 288 GB HBM3E per (unpartitioned) GPU, 256 CUs
        if node.properties.get("num_xcc", 0) >= 8:
            assert node.vram_bytes > 280 * 1024**3
            assert node.cu_count == 256
    # gpurun containers cgroup-mask peer GPUs' kfd nodes: only kfd-backed
    # devices carry the devID join
    backed = [d for d in devs.values() if d.kfd_backed]
    assert backed, "no kfd-backed device on a GPU box"
    for d in backed:
        assert d.render_d >= 128
        assert d.dev_id, f"devID join failed for {d.id}"


def test_advertised_vs_present(live_devices):
    import torch

    _, devs = live_devices
    present = torch.cuda.device_count()
    # schedulable (kfd-backed) devices must match what HIP sees — whole
    # GPUs in SPX, partitions in CPX (each partition is one HIP device);
    # cgroup-masked peers are advertised Unhealthy and don't count
    schedulable = sum(1 for d in devs.values() if d.kfd_backed)
    assert schedulable == present, (
        f"kfd walk found {schedulable} schedulable devices, torch sees {present}"
    )


def test_drmctl_ioctls(live_devices):
    from k8s_device_plugin_amd.native import load_drmctl

    _, devs = live_devices
    drm = load_drmctl(required=True)
    backed = [d for d in devs.values() if d.kfd_backed]
    d = sorted(backed, key=lambda x: x.render_d)[0]
    dev_path = f"/dev/dri/renderD{d.render_d}"

    assert drm.dev_functional(dev_path)
    info = drm.query_device_info(dev_path)
    assert info["device_id"] > 0
    assert info["family"] > 0
    assert info["cu_active_number"] > 0
    fw = drm.query_firmware(dev_path)
    # at least the GFX blocks must report non-zero firmware on a live GPU
    assert any(v > 0 for v in fw["firmware"].values()), fw
    vram = drm.query_vram(dev_path)
    assert vram["vram_size"] > 1 << 30


def test_deep_health_probe():
    _require_gpu()
    from k8s_device_plugin_amd.native import deep_health_probe

    probe = deep_health_probe(device=0, hbm_bytes=1 << 30)
    assert probe["wavefront_size"] == 64
    assert probe["wave_ok"]
    assert probe["mfma_ok"], probe
    assert probe["lds_ok"], probe
    assert probe["hbm_copy_ok"], probe
    # healthy now also implies the DVFS-aware performance floors held
    # (1000 TF/s MFMA, 3800 GB/s HBM) — a healthy MI355X must clear them
    # with margin, and the floors fields must be reported
    assert probe["healthy"]
    assert probe["floor_violations"] == [], probe
    assert probe["floors"]["mfma_tflops"] > 0
    assert probe["mfma_tflops"] > probe["floors"]["mfma_tflops"], probe
    assert probe["hbm_gbps"] > probe["floors"]["hbm_gbps"], probe
    # an absurd floor must flip the verdict on the same hardware
    degraded = deep_health_probe(device=0, hbm_bytes=1 << 28,
                                 mfma_floor_tflops=10_000_000)
    assert not degraded["healthy"]
    assert degraded["floor_violations"], degraded


@pytest.mark.parametrize("hbm_bytes", [
    16,                        # n = 1: one thread, tail path only
    16 * 31,                   # n = 31: sample windows overlap, none may pass n
    16 * (3 * 262144 + 5),     # minimum 1024-block grid: 5 threads 4-wide, rest tail
    16 * (4 * 262144 + 7),     # ceil(n/1024) blocks: 4-wide and tail threads mixed
])
def test_deep_probe_hbm_copy_odd_sizes(hbm_bytes):
    """The copy's head, middle and end are checked component by component
    at sizes where the one-shot kernel's 4-wide and tail paths mix; floors
    are off so that only correctness decides."""
    _require_gpu()
    from k8s_device_plugin_amd.native import deep_health_probe

    probe = deep_health_probe(device=0, hbm_bytes=hbm_bytes,
                              mfma_floor_tflops=0, hbm_floor_gbps=0)
    assert probe["hbm_copy_ok"], probe
    assert probe["healthy"], probe
    assert probe["hbm_bytes_tested"] == hbm_bytes


def test_smoke_entry():
    _require_gpu()
    sys.path.insert(0, REPO)
    import __graft_entry__ as entry

    entry.smoke()


def test_bench_single_gpu():
    _require_gpu()
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--steps", "50",
         "--warmup", "5"],
        capture_output=True, text=True, timeout=300,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    line = out.stdout.strip().splitlines()[-1]
    rec = json.loads(line)
    assert rec["config"]["sysfs"] == "live"
    assert rec["config"]["present_gpus"] >= 1
    assert rec["config"]["advertised_gpus"] >= 1
    assert rec["value"] > 0


def test_firmware_ioctl_vs_debugfs(live_devices):
    """Cross-check ioctl firmware versions against debugfs when readable
    (reference: amdgpu_test.go:45-75)."""
    from k8s_device_plugin_amd.native import load_drmctl
    from k8s_device_plugin_amd.topology.firmware import (
        debugfs_firmware_path,
        parse_debugfs_firmware,
    )

    _, devs = live_devices
    drm = load_drmctl(required=True)
    d = sorted((x for x in devs.values() if x.kfd_backed),
               key=lambda x: x.render_d)[0]
    fw = drm.query_firmware(f"/dev/dri/renderD{d.render_d}")
    feat_dbg, fw_dbg = parse_debugfs_firmware(debugfs_firmware_path(d.card))
    if not fw_dbg:
        pytest.skip("debugfs not readable in this container")
    for blk in ("MEC", "RLC", "SDMA0"):
        if blk in fw_dbg and fw["firmware"][blk]:
            assert fw["firmware"][blk] == fw_dbg[blk], blk


def test_allocate_paths_are_real_devices(live_devices):
    """The device nodes Allocate returns must exist and answer ioctls —
    validates the full path kubelet would inject into a container."""
    from k8s_device_plugin_amd.native import load_drmctl
    from k8s_device_plugin_amd.plugin import AMDGPUPlugin
    from k8s_device_plugin_amd.protos import deviceplugin as dp

    paths, devs = live_devices
    drm = load_drmctl(required=True)
    plugin = AMDGPUPlugin(resource="gpu", paths=paths)
    plugin.start()
    backed = sorted((d for d in devs.values() if d.kfd_backed),
                    key=lambda d: d.id)
    req = dp.AllocateRequest()
    req.container_requests.add().devices_ids.append(backed[0].id)
    resp = plugin.Allocate(req, None)
    specs = [s.host_path for s in resp.container_responses[0].devices]
    assert "/dev/kfd" in specs
    render = [p for p in specs if "renderD" in p]
    assert render and os.path.exists(render[0])
    assert drm.dev_functional(render[0])


def test_labeller_on_live_sysfs(live_devices):
    """Label generation on the real MI355X: gfx950 values end-to-end.

    Partition-mode-dependent values (vram/cu/simd per schedulable device)
    are derived from the live kfd tree so the test holds in SPX and CPX
    alike; identity values are asserted fixed."""
    from k8s_device_plugin_amd.labeller import generate_labels
    from k8s_device_plugin_amd.labeller.labels import LABEL_KINDS
    from k8s_device_plugin_amd.topology import KFDTopology, SysPaths

    paths, devs = live_devices
    labels = generate_labels({k: True for k in LABEL_KINDS}, SysPaths("/"))

    # identity facts: fixed for MI355X regardless of partition mode
    assert labels["amd.com/gpu.device-id"] == "75a3"
    assert labels["amd.com/gpu.family"] == "AI"
    assert "MI355" in labels["amd.com/gpu.product-name"]
    assert labels["amd.com/gpu.compute-partitioning-supported"] in ("true", "false")

    # mode-dependent values must match the first kfd-backed physical GPU
    topo = KFDTopology.load(paths)
    backed = next(d for d in devs.values() if d.kfd_backed and not d.is_partition)
    node = topo.node_by_render_minor(backed.render_d)
    g = round(node.vram_bytes // (1024 * 1024) / 1024)
    assert labels["amd.com/gpu.vram"] == f"{g}G"
    assert labels["amd.com/gpu.cu-count"] == str(node.cu_count)
    assert labels["amd.com/gpu.simd-count"] == str(node.simd_count)
    # xGMI hive tagging from the real kfd hive_id
    if node.hive_id:
        assert int(labels["amd.com/gpu.xgmi-hive-count"]) >= 1
        assert f"{node.hive_id:x}" in "".join(
            k for k in labels if "xgmi-hive" in k
        ) or labels.get("amd.com/gpu.xgmi-hive") == f"{node.hive_id:x}"
    if backed.compute_partition == "spx":
        assert labels["amd.com/gpu.vram"] == "288G"
        assert labels["amd.com/gpu.cu-count"] == "256"
        assert labels["amd.com/gpu.compute-memory-partition"].startswith("spx_")
    # firmware labels come from the raw-ioctl shim on a live box
    fw_labels = [k for k in labels if k.startswith("beta.amd.com/gpu.firmware.")]
    assert fw_labels, "expected firmware labels via drmctl ioctls"


def test_prestart_probe_live(live_devices):
    """--prestart-probe against the real renderD node via the native server."""
    import grpc
    import tempfile

    from k8s_device_plugin_amd.plugin import AMDGPUPlugin
    from k8s_device_plugin_amd.plugin.native_server import NativePluginServer
    from k8s_device_plugin_amd.protos import deviceplugin as dp

    paths, devs = live_devices
    plugin = AMDGPUPlugin(resource="gpu", paths=paths, prestart_probe=True)
    plugin.start()
    with tempfile.TemporaryDirectory() as tmp:
        srv = NativePluginServer(plugin, f"{tmp}/ps.sock")
        srv.start()
        try:
            ch = grpc.insecure_channel(f"unix://{tmp}/ps.sock")
            stub = dp.DevicePluginStub(ch)
            backed = sorted(d.id for d in devs.values() if d.kfd_backed)
            req = dp.PreStartContainerRequest()
            req.devices_ids.extend(backed[:1])
            assert stub.PreStartContainer(req, timeout=5) is not None
            opts = stub.GetDevicePluginOptions(dp.Empty(), timeout=5)
            assert opts.pre_start_required
            ch.close()
        finally:
            srv.stop()


def test_xgmi_p2p_bandwidth():
    """GPU->GPU copy bandwidth over xGMI (needs >=2 visible GPUs; the
    allocator's hive packing exists to keep jobs on these links)."""
    _require_gpu()
    from k8s_device_plugin_amd.native import load_healthprobe

    hp = load_healthprobe(required=True)
    n = hp.device_count()
    if n < 2:
        pytest.skip(f"only {n} GPU(s) visible")
    r = hp.p2p_bandwidth(0, 1, 1 << 30)
    assert r["peer_access"], r
    # one xGMI point-to-point link is ~153 GB/s class, but a single
    # hipMemcpyPeer stream may be SDMA-engine-limited well below the link
    # rate; assert a conservative floor and report the measured value
    assert r["gbps"] > 15, f"p2p bandwidth {r['gbps']:.0f} GB/s: link broken?"
    print(f"p2p 0->1: {r['gbps']:.0f} GB/s")


def test_full_stack_daemon_live(tmp_path):
    """The real CLI daemon on live sysfs with pulse + CDI + metrics:
    registration, stream, allocate, health refresh, CDI spec, metrics."""
    _require_gpu()
    import json as _json
    import signal
    import socket as _socket
    import subprocess
    import urllib.request

    from k8s_device_plugin_amd.testing.stub_kubelet import StubKubelet
    from k8s_device_plugin_amd.protos import deviceplugin as dp

    with _socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        mport = s.getsockname()[1]

    dp_dir = str(tmp_path / "dp")
    cdi_dir = str(tmp_path / "cdi")
    kubelet = StubKubelet(dp_dir).start()
    proc = subprocess.Popen(
        [sys.executable, "-m", "k8s_device_plugin_amd.cli",
         "--pulse", "1", "--kubelet-dir", dp_dir,
         "--cdi", "--cdi-dir", cdi_dir,
         "--metrics-port", str(mport)],
        cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
    )
    try:
        reg = kubelet.wait_for_registration(timeout=60)
        assert reg.resource_name == "amd.com/gpu"
        stub = kubelet.connect(reg.endpoint)
        call = stub.ListAndWatch(dp.Empty())
        it = iter(call)
        first = next(it)
        healthy = [d.ID for d in first.devices if d.health == "Healthy"]
        assert healthy
        second = next(it)  # pulse=1 refresh
        assert {d.ID for d in second.devices} == {d.ID for d in first.devices}

        req = dp.AllocateRequest()
        req.container_requests.add().devices_ids.append(healthy[0])
        resp = stub.Allocate(req, timeout=10)
        car = resp.container_responses[0]
        assert any("/dev/kfd" == s.host_path for s in car.devices)
        assert [c.name for c in car.cdi_devices] == [
            f"amd.com/gpu={healthy[0]}"
        ]

        spec = _json.load(open(os.path.join(cdi_dir, "amd.com-gpu.json")))
        assert any(d["name"] == healthy[0] for d in spec["devices"])

        body = urllib.request.urlopen(
            f"http://127.0.0.1:{mport}/metrics", timeout=10
        ).read().decode()
        assert "amdgpu_dp_allocate_total" in body
        call.cancel()
        proc.send_signal(signal.SIGTERM)
        assert proc.wait(timeout=20) == 0
    finally:
        if proc.poll() is None:
            proc.kill()
            proc.wait()
        kubelet.stop()


def test_mfma_elementwise_vs_torch():
    """Element-wise verification of v_mfma_f32_16x16x32_bf16 against a
    PyTorch fp32 matmul through the CDNA4 lane->element maps
    (cdna_hip_programming.md §3: D col=lane&15, row=(lane>>4)*4+reg;
    A/B 8 elements per lane along K).  All values are small ints, exact
    in bf16 and f32, so the comparison is bitwise."""
    _require_gpu()
    import torch

    from k8s_device_plugin_amd.native import load_healthprobe

    hp = load_healthprobe(required=True)
    raw = hp.mfma_probe_raw(0)

    # reconstruct A (16x32) and B (32x16) from the kernel's lane patterns
    A = torch.zeros(16, 32)
    B = torch.zeros(32, 16)
    for lane in range(64):
        for r in range(8):
            k = (lane >> 4) * 8 + r
            A[lane & 15, k] = ((lane * 8 + r) % 7) - 3
            B[k, lane & 15] = ((lane * 5 + r * 3) % 11) - 5
    D = A @ B  # fp32 reference, exact for these integers

    mismatches = []
    for lane in range(64):
        for reg in range(4):
            row = (lane >> 4) * 4 + reg
            col = lane & 15
            got = raw["pass2"][lane * 4 + reg]
            want = float(D[row, col])
            if got != want:
                mismatches.append((lane, reg, row, col, got, want))
    assert not mismatches, (
        f"{len(mismatches)}/256 MFMA elements differ from the torch "
        f"reference; first 8: {mismatches[:8]}"
    )

    # pass 0/1 invariants still hold on the raw path
    assert all(v == 16.0 for v in raw["pass0"])


def test_partitionctl_read_live(live_devices):
    """Read-only partition state on live sysfs (writes are forbidden on
    shared boxes — the gate refuses without AMDXDP_ALLOW_REPARTITION)."""
    import os

    from k8s_device_plugin_amd.topology import (
        PartitionError,
        SysPaths,
        available_partition_modes,
        current_partition_modes,
        set_partition_mode,
    )

    paths = SysPaths("/")
    cur = current_partition_modes(paths)
    assert cur, "no amdgpu PCI devices visible"
    for addr, (comp, mem) in cur.items():
        # live MI355X reports real modes (SPX/CPX..., NPS1...)
        assert comp in ("SPX", "DPX", "TPX", "QPX", "CPX", ""), (addr, comp)
        assert mem.startswith("NPS") or mem == "", (addr, mem)
    comp_avail, mem_avail = available_partition_modes(paths)
    # MI355X supports compute partitioning; the capability files exist
    assert "SPX" in comp_avail or comp_avail == []
    # the safety gate must refuse writes on this shared box
    os.environ.pop("AMDXDP_ALLOW_REPARTITION", None)
    try:
        set_partition_mode(paths, compute="SPX", allow=True)
        raise AssertionError("gate did not refuse")
    except PartitionError:
        pass


def test_deep_probe_heartbeat_live(live_devices):
    """--deep-probe-every on real hardware: the heartbeat deep check runs
    the MFMA/LDS/HBM probe against the live GPU and keeps it Healthy."""
    from k8s_device_plugin_amd.plugin import AMDGPUPlugin
    from k8s_device_plugin_amd.protos import deviceplugin as dp
    from k8s_device_plugin_amd.topology import SysPaths

    class _Ctx:
        def is_active(self):
            return True

    plugin = AMDGPUPlugin(resource="gpu", paths=SysPaths("/"),
                          deep_probe_every=1)
    plugin.start()
    stream = plugin.ListAndWatch(dp.Empty(), _Ctx())
    next(stream)
    plugin.heartbeat()  # runs the real probe on every kfd-backed GPU
    resp = next(stream)
    backed = {d.id for d in plugin.devices.values() if d.kfd_backed}
    health = {d.ID: d.health for d in resp.devices}
    for did in backed:
        assert health[did] == "Healthy", (did, plugin._deep_failed)
    assert not plugin._deep_failed
    plugin.stop()


def test_hip_ordinal_pci_mapping(live_devices):
    """The plugin's device->HIP-ordinal mapping must go through the
    runtime's PCI bus ids (exact match), not enumeration-order guessing."""
    import torch

    from k8s_device_plugin_amd.native import load_healthprobe
    from k8s_device_plugin_amd.plugin import AMDGPUPlugin
    from k8s_device_plugin_amd.topology import SysPaths

    mod = load_healthprobe(required=True)
    bus_ids = mod.pci_bus_ids()
    assert len(bus_ids) == torch.cuda.device_count()
    assert all(b for b in bus_ids), bus_ids

    plugin = AMDGPUPlugin(resource="gpu", paths=SysPaths("/"))
    plugin.start()
    backed = [d for d in plugin.devices.values() if d.kfd_backed]
    for d in backed:
        ordinal = plugin._hip_ordinal(d)
        assert 0 <= ordinal < len(bus_ids)
        assert bus_ids[ordinal].lower().replace(".", ":") == \
            d.dev_id.lower().replace(".", ":")
    plugin.stop()
