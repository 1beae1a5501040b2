import itertools
import os
import pathlib
import shutil
import sys
import tempfile

import pytest

# Make the repo root importable regardless of how pytest is invoked.
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pytest_configure(config):
    config.addinivalue_line(
        "markers", "gpu: test requires a real AMD GPU (run on an MI355X box)"
    )
    # build the CPU-buildable native extensions if missing so a fresh
    # checkout passes without a separate build step (g++ only; the HIP
    # probe needs hipcc and is attempted best-effort)
    from k8s_device_plugin_amd.native import build as nb

    nb.build_drmctl()
    nb.build_fastserver()
    nb.build_h2tool()
    try:
        nb.build_healthprobe()
    except Exception:
        pass  # no hipcc on this machine; gpu-marked tests need it anyway


class _ShortTmpFactory:
    """Stand-in for pytest's TempPathFactory (mktemp/getbasetemp only) that
    hands out <short root>/dpt-XXXXXXXX/<basename>N directories.

    Most tests here bind unix sockets under their temporary directory, and
    pytest's own base (<tmp>/pytest-of-<user>/pytest-N/<test name>N/) can
    use up most of sun_path's 107 bytes before the test adds
    "device-plugins/kubelet.sock": the suite passed or failed with the
    length of the user name and of $TMPDIR."""

    def __init__(self):
        from k8s_device_plugin_amd.testing.sockdir import short_tmp_root

        self._base = pathlib.Path(
            tempfile.mkdtemp(prefix="dpt-", dir=short_tmp_root())
        )
        self._count = itertools.count()

    def getbasetemp(self) -> pathlib.Path:
        return self._base

    def mktemp(self, basename: str, numbered: bool = True) -> pathlib.Path:
        name = f"{basename}{next(self._count)}" if numbered else basename
        path = self._base / name
        path.mkdir()
        return path

    def cleanup(self) -> None:
        shutil.rmtree(self._base, ignore_errors=True)


@pytest.fixture(scope="session")
def tmp_path_factory():
    factory = _ShortTmpFactory()
    yield factory
    factory.cleanup()


@pytest.fixture
def tmp_path(tmp_path_factory):
    path = tmp_path_factory.mktemp("t")
    yield path
    shutil.rmtree(path, ignore_errors=True)


@pytest.fixture
def fake_mi355x_8(tmp_path):
    """8*MI355X SPX/NPS1 node, single xGMI hive."""
    from k8s_device_plugin_amd.testing.fakesysfs import build_mi355x_node

    return build_mi355x_node(str(tmp_path / "root"))


@pytest.fixture
def fake_mi355x_cpx(tmp_path):
    """8*MI355X in CPX/NPS2: 8 physical GPUs x 8 partitions = 64 devices."""
    from k8s_device_plugin_amd.testing.fakesysfs import build_mi355x_node

    return build_mi355x_node(
        str(tmp_path / "root"),
        partitions_per_gpu=8,
        compute_partition="CPX",
        memory_partition="NPS2",
    )
