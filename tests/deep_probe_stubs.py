"""What the deep-probe policy tests share: the stub-module installer, the
module as it was before any sweep, the 2 GPU x 4 partition plugin and the
gauge reader.  A plain module, imported like tests/valu_reference.py; result
builders and bad entries differ per sweep and stay in their files.
"""

import types

import pytest

import k8s_device_plugin_amd.native as native
from k8s_device_plugin_amd.plugin import AMDGPUPlugin
from k8s_device_plugin_amd.testing.fakesysfs import build_mi355x_node

SWEEP_ENVS = (
    native.CU_SWEEP_ENV, native.CU_SWEEP_INJECT_ENV, native.CU_SWEEP_EXTRA_ENV,
    native.LDS_SWEEP_ENV, native.LDS_SWEEP_INJECT_ENV,
    native.VALU_SWEEP_ENV, native.VALU_SWEEP_INJECT_ENV, native.HBM_SCRUB_ENV,
)


class Ctx:
    def is_active(self):
        return True


def dev_root(tmp_path):
    d = tmp_path / "dev"
    d.mkdir(exist_ok=True)
    (d / "kfd").touch()
    return str(d)


class ProbeOnlyStub:
    """The module as it was before the sweeps: run_probe and nothing else."""

    def __init__(self):
        self.calls = []

    def run_probe(self, device=0, hbm_bytes=0):
        self.calls.append(device)
        return {"wave_ok": True, "mfma_ok": True, "lds_ok": True,
                "hbm_copy_ok": True, "mfma_tflops": 2000.0,
                "hbm_gbps": 6200.0, "healthy": True}


@pytest.fixture
def stub_probe(monkeypatch):
    """Clears every sweep's environment variables; the returned installer
    makes native.load_healthprobe hand out the given module."""
    for env in SWEEP_ENVS:
        monkeypatch.delenv(env, raising=False)

    def _install(mod):
        monkeypatch.setattr(native, "load_healthprobe",
                            lambda required=None: mod)
        return mod
    return _install


def cpx_plugin(tmp_path, stub_probe, make_stub, **kwargs):
    """2 physical GPUs x 4 partitions; HIP ordinals 0-3 are GPU 0's
    partitions and 4-7 GPU 1's (the same PCI bus id four times each).
    make_stub(bus_ids) builds the module to install."""
    fs = build_mi355x_node(str(tmp_path / "n"), n_gpus=2, partitions_per_gpu=4)
    plugin = AMDGPUPlugin(resource="gpu", paths=fs.paths,
                          dev_root=dev_root(tmp_path), **kwargs)
    plugin.start()
    phys = sorted({d.dev_id for d in plugin.devices.values()})
    assert len(phys) == 2
    mod = stub_probe(make_stub([phys[0]] * 4 + [phys[1]] * 4))
    return plugin, mod, phys


def gauge(plugin, name):
    """[(labels, value)] of one metric family of a one-plugin manager."""
    from k8s_device_plugin_amd.plugin.metrics import _ManagerCollector

    manager = types.SimpleNamespace(
        plugins={"gpu": types.SimpleNamespace(plugin=plugin, native=False)})
    families = {f.name: f for f in _ManagerCollector(manager).collect()}
    return [(s.labels, s.value) for s in families[name].samples]
