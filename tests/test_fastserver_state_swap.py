"""Replacing the allocator state under a live native server.

The server tabulates the state once per `set_allocator_state` and keeps one
scratch for every search it runs; a heartbeat that finds another device set
swaps the tables under it.  After each swap every answer must be the Python
policy's for the state then loaded, nothing left over from the one before.
"""

import grpc

from k8s_device_plugin_amd.allocator import AllocationError, BestEffortPolicy
from k8s_device_plugin_amd.plugin import AMDGPUPlugin
from k8s_device_plugin_amd.plugin.native_server import NativePluginServer
from k8s_device_plugin_amd.protos import deviceplugin as dp
from k8s_device_plugin_amd.testing.fakesysfs import build_mi355x_node
from k8s_device_plugin_amd.topology import KFDTopology, discover_gpus


def _ask(stub, available, required, size):
    """The server's id list, or None where it answers INVALID_ARGUMENT."""
    req = dp.PreferredAllocationRequest()
    cr = req.container_requests.add()
    cr.available_deviceIDs.extend(available)
    cr.must_include_deviceIDs.extend(required)
    cr.allocation_size = size
    try:
        resp = stub.GetPreferredAllocation(req, timeout=10)
    except grpc.RpcError as e:
        assert e.code() == grpc.StatusCode.INVALID_ARGUMENT, e
        return None
    return list(resp.container_responses[0].deviceIDs)


def _want(policy, available, required, size):
    try:
        return policy.allocate(available, required, size)
    except AllocationError:
        return None


def test_answers_follow_the_loaded_state(tmp_path, fake_mi355x_cpx):
    plugin = AMDGPUPlugin(resource="gpu", paths=fake_mi355x_cpx.paths)
    plugin.start()
    big = plugin.allocator
    ids64 = sorted(plugin.devices)
    assert len(ids64) == 64

    fs2 = build_mi355x_node(str(tmp_path / "two"), n_gpus=2)
    topo2 = KFDTopology.load(fs2.paths)
    devs2 = discover_gpus(fs2.paths, topology=topo2)
    small = BestEffortPolicy()
    small.init(devs2.values(), topology=topo2)
    ids2 = sorted(devs2)
    assert len(ids2) == 2

    requests = [
        (ids64, [], 30),
        (ids64, [], 63),
        (ids64, [], 4),
        (ids64[3:40], [ids64[5]], 9),
        (ids64[::3], [], 1),
        (ids2, [], 1),
        (list(reversed(ids2)), [], 1),
        (ids2, [ids2[1]], 1),
        (ids2 + ids64[:6], [], 3),
        (ids2 + ["not-a-dev"], [ids2[1]], 2),
    ]

    srv = NativePluginServer(plugin, str(tmp_path / "swap.sock"))
    srv.start()
    channel = grpc.insecure_channel(f"unix://{srv.socket_path}")
    stub = dp.DevicePluginStub(channel)
    try:
        for policy in (big, small, big, small, big):
            srv._srv.set_allocator_state(*policy.export_state())
            answered = 0
            for available, required, size in requests:
                got = _ask(stub, available, required, size)
                assert got == _want(policy, available, required, size), \
                    (len(policy._devices), len(available), required, size)
                answered += got is not None
            # every state answers some of these, the small one not all
            assert answered >= 3
            assert policy is big or answered < len(requests)
    finally:
        channel.close()
        srv.stop()
