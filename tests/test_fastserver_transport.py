"""The native server's syscall budget per RPC, and what happens when the
socket will not take a response.

Both tests read the transport counters of `stats()` (`socket_writes_total`,
`socket_reads_total`, `socket_write_would_block_total`) around traffic from
the raw HTTP/2 client, which puts each request on the wire with one send.
"""

import struct
import time

from k8s_device_plugin_amd.plugin import AMDGPUPlugin
from k8s_device_plugin_amd.plugin.native_server import NativePluginServer
from k8s_device_plugin_amd.protos import deviceplugin as dp
from k8s_device_plugin_amd.testing.h2raw import (
    DATA,
    FLAG_END_HEADERS,
    FLAG_END_STREAM,
    HEADERS,
    H2Conn,
    frame,
    grpc_frame,
)

ALLOCATE = "/v1beta1.DevicePlugin/Allocate"
SETTINGS_INITIAL_WINDOW_SIZE = 4
MAX_WINDOW = 2**31 - 1


def _serve(tmp_path, fs):
    plugin = AMDGPUPlugin(resource="gpu", paths=fs.paths)
    plugin.start()
    srv = NativePluginServer(plugin, str(tmp_path / "tr.sock"))
    srv.start()
    return plugin, srv


def _connect(srv):
    """A connection whose flow-control windows (every stream's and the
    connection's) are as wide as HTTP/2 allows and are never topped up, so
    the client sends nothing but requests.  Returns once the server has
    read and answered everything the handshake put on the wire."""
    conn = H2Conn(srv.socket_path,
                  settings=[(SETTINGS_INITIAL_WINDOW_SIZE, MAX_WINDOW)])
    conn.auto_window_update = False
    conn.window_update(MAX_WINDOW - 65535, 0)
    # our ack of the server's SETTINGS goes out when we read them ...
    assert conn.wait_now(lambda: conn.settings_acked and conn.server_settings)
    # ... and a connection is served in order: once this PING is answered,
    # the server has read that ack and written all it had to write
    conn.ping(b"settled!")
    assert conn.wait_now(lambda: b"settled!" in conn.pings_acked)
    return conn


def _allocate_bytes(conn, device_ids):
    """(stream id, one buffer holding the whole Allocate request)."""
    req = dp.AllocateRequest()
    req.container_requests.add().devices_ids.extend(device_ids)
    sid = conn.next_stream_id()
    block = conn.encode_headers([
        (":method", "POST"),
        (":scheme", "http"),
        (":path", ALLOCATE),
        (":authority", "localhost"),
        ("content-type", "application/grpc"),
        ("te", "trailers"),
    ])
    return sid, (frame(HEADERS, FLAG_END_HEADERS, sid, block) +
                 frame(DATA, FLAG_END_STREAM, sid,
                       grpc_frame(req.SerializeToString())))


def test_one_write_and_one_read_per_unary_rpc(tmp_path, fake_mi355x_8):
    """K awaited Allocate calls cost the server K writes and K reads.

    A response is three frames (HEADERS, DATA, trailer HEADERS); sent one
    write() each, and with a second read() per request just to see EAGAIN,
    that would be 3K writes and 2K reads.

    Allowance: 2 calls each way.  After _connect() nothing but the K
    requests and their responses is due on this connection: both SETTINGS
    acks are through, the client sends no WINDOW_UPDATE, and the server
    owes none (it tops a window up after half of 65,535 request bytes; K
    requests are about 12 KB).  What remains is the kernel's freedom to
    hand over a stream socket's bytes in two pieces, which for messages of
    under 200 bytes it does not use; 2 leaves room for it without hiding a
    per-RPC extra, which would show up K = 200 times."""
    K, ALLOWANCE = 200, 2
    plugin, srv = _serve(tmp_path, fake_mi355x_8)
    try:
        conn = _connect(srv)
        ids = sorted(plugin.devices)
        before = srv._srv.stats()
        for i in range(K):
            sid, data = _allocate_bytes(conn, [ids[i % len(ids)]])
            conn.send_raw(data)
            st = conn.stream(sid)
            assert conn.wait_now(lambda: st.ended), f"no response to call {i}"
            assert st.grpc_status() == "0"
            resp = dp.AllocateResponse.FromString(st.grpc_messages()[0])
            assert len(resp.container_responses[0].devices) == 3
        after = srv._srv.stats()
        conn.close()
    finally:
        srv.stop()
    assert after["allocate_total"] - before["allocate_total"] == K
    writes = after["socket_writes_total"] - before["socket_writes_total"]
    reads = after["socket_reads_total"] - before["socket_reads_total"]
    print(f"{K} RPCs: {writes} writes, {reads} reads")
    assert K <= writes <= K + ALLOWANCE
    assert K <= reads <= K + ALLOWANCE
    assert (after["socket_write_would_block_total"] ==
            before["socket_write_would_block_total"])


def test_back_pressure_keeps_bytes_and_order(tmp_path, fake_mi355x_cpx):
    """64 pipelined Allocate calls for all 64 CPX devices, nothing read
    until the server has run into the full socket: 64 responses of 5.6 KB,
    over 350 KB, against a unix-socket buffer of about 208 KB plus the 64 KB
    the server gathers.  Every response must arrive whole and equal to the
    one the same request gets alone.

    64 is as many as a client that does not read may send.  Request DATA
    counts against the server's receive window of 65,535 bytes, and the
    WINDOW_UPDATE that would reopen it queues up behind the responses the
    socket will not take; 64 requests are 62 KB of DATA.  More (128 calls
    with two containers each would make 1.4 MB of responses) ends in
    GOAWAY(FLOW_CONTROL_ERROR), as HTTP/2 prescribes, whatever the server
    does with its writes."""
    N = 64
    plugin, srv = _serve(tmp_path, fake_mi355x_cpx)
    try:
        ids = sorted(plugin.devices)
        assert len(ids) == 64

        alone = _connect(srv)
        sid, data = _allocate_bytes(alone, ids)
        alone.send_raw(data)
        want = alone.stream(sid)
        assert alone.wait_now(lambda: want.ended)
        assert want.grpc_status() == "0"
        assert len(dp.AllocateResponse.FromString(want.grpc_messages()[0])
                   .container_responses[0].devices) == 1 + 2 * 64
        alone.close()
        assert N * len(want.data) > 350_000
        assert N * (len(data) - 9) < 65_535  # DATA payloads, HEADERS aside

        conn = _connect(srv)
        before = srv._srv.stats()
        sids = []
        for _ in range(N):
            sid, data = _allocate_bytes(conn, ids)
            conn.send_raw(data)
            sids.append(sid)

        def blocked():
            return (srv._srv.stats()["socket_write_would_block_total"] >
                    before["socket_write_would_block_total"])

        # without this the test would not have reached the path it is about
        deadline = time.monotonic() + 10
        while not blocked() and time.monotonic() < deadline:
            time.sleep(0.001)
        assert blocked(), "the server never met a full socket"

        streams = [conn.stream(s) for s in sids]
        assert conn.wait_now(lambda: all(s.ended for s in streams), timeout=30)
        after = srv._srv.stats()
        conn.close()
    finally:
        srv.stop()
    assert after["allocate_total"] - before["allocate_total"] == N
    for i, s in enumerate(streams):
        assert s.rst is None and s.grpc_status() == "0", (i, s.trailers)
        assert s.data == want.data, f"response {i} differs"
        assert (struct.unpack("!I", s.data[1:5])[0] == len(s.data) - 5)
    # gathered, not frame by frame: far fewer writes than the ~3 frames of
    # up to 16 KB per response would take one at a time
    writes = after["socket_writes_total"] - before["socket_writes_total"]
    print(f"{N * len(want.data)} bytes in {writes} writes")
    assert writes < 3 * N
