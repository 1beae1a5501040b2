"""Plugin lifecycle manager: serve, register, re-register on kubelet restart.

Replaces the reference's vendored dpm manager (reference:
vendor/github.com/kubevirt/device-plugin-manager/pkg/dpm/manager.go:41-193,
plugin.go:50-162): one gRPC server per resource on
/var/lib/kubelet/device-plugins/amd.com_<resource>, registration with the
kubelet Registration service, and a watch on kubelet.sock that re-registers
every plugin when the kubelet restarts (the dpm fsnotify path, expressed as
an inode-change poll, which also survives the rename-over dance fsnotify
misses).
"""

from __future__ import annotations

import logging
import os
import threading
import time
from concurrent.futures import ThreadPoolExecutor
from typing import Callable, Dict, List, Optional

from ..protos import deviceplugin as dp
from .server import AMDGPUPlugin

log = logging.getLogger(__name__)


class _PluginInstance:
    def __init__(self, resource: str, plugin: AMDGPUPlugin, socket_path: str):
        self.resource = resource
        self.plugin = plugin
        self.socket_path = socket_path
        self.server = None  # grpc.Server or NativePluginServer
        self.native = False

    @property
    def endpoint(self) -> str:
        return os.path.basename(self.socket_path)


class PluginManager:
    def __init__(
        self,
        plugin_factory: Callable[[str], AMDGPUPlugin],
        namespace: str = dp.RESOURCE_NAMESPACE,
        device_plugin_path: str = dp.DEVICE_PLUGIN_PATH,
        kubelet_socket: Optional[str] = None,
        watch_interval: float = 0.5,
        server_impl: str = "native",
    ):
        """server_impl: "native" (C++/nghttp2 fast server; falls back to
        python when the extension or libnghttp2 is unavailable) or
        "python" (grpc.Server)."""
        self.plugin_factory = plugin_factory
        self.server_impl = server_impl
        self.namespace = namespace
        self.device_plugin_path = device_plugin_path
        self.kubelet_socket = kubelet_socket or os.path.join(
            device_plugin_path, "kubelet.sock"
        )
        self.watch_interval = watch_interval
        self.plugins: Dict[str, _PluginInstance] = {}
        self._stop = threading.Event()
        self._watch_thread: Optional[threading.Thread] = None
        self._lock = threading.Lock()

    # ---- plugin serving ----

    def start_resource(self, resource: str) -> _PluginInstance:
        import grpc

        with self._lock:
            if resource in self.plugins:
                return self.plugins[resource]
            socket_path = os.path.join(
                self.device_plugin_path, f"{self.namespace}_{resource}"
            )
            plugin = self.plugin_factory(resource)
            plugin.on_stream_lost = lambda: self._reregister_async(resource)
            plugin.start()

            if os.path.exists(socket_path):
                os.unlink(socket_path)

            server = None
            native = False
            if self.server_impl == "native":
                try:
                    from .native_server import NativePluginServer

                    server = NativePluginServer(plugin, socket_path)
                    server.start()
                    native = True
                    log.info("%s: serving via native fast server", resource)
                except Exception as e:
                    log.warning(
                        "%s: native server unavailable (%s); falling back to "
                        "python grpc", resource, e,
                    )
                    server = None
            if server is None:
                # Allocate/GetPreferredAllocation are tiny; a few workers
                # keep the ListAndWatch streams responsive.
                server = grpc.server(ThreadPoolExecutor(max_workers=8))
                dp.add_device_plugin_servicer(server, plugin)
                server.add_insecure_port(f"unix://{socket_path}")
                server.start()

            inst = _PluginInstance(resource, plugin, socket_path)
            inst.server = server
            inst.native = native
            self.plugins[resource] = inst
        self.register(inst)
        return inst

    def register(self, inst: _PluginInstance, retries: int = 5) -> bool:
        """Register one plugin with the kubelet (reference: dpm/plugin.go:127-162)."""
        import grpc

        req = dp.RegisterRequest(
            version=dp.VERSION,
            endpoint=inst.endpoint,
            resource_name=f"{self.namespace}/{inst.resource}",
        )
        opts = inst.plugin.GetDevicePluginOptions(dp.Empty(), None)
        req.options.CopyFrom(opts)

        for attempt in range(retries):
            try:
                with grpc.insecure_channel(f"unix://{self.kubelet_socket}") as ch:
                    dp.RegistrationStub(ch).Register(req, timeout=5)
                log.info(
                    "registered %s/%s at endpoint %s",
                    self.namespace, inst.resource, inst.endpoint,
                )
                return True
            except grpc.RpcError as e:
                log.warning(
                    "registration attempt %d for %s failed: %s",
                    attempt + 1, inst.resource, e,
                )
                time.sleep(min(2 ** attempt * 0.1, 2.0))
        return False

    def _reregister_async(self, resource: str) -> None:
        inst = self.plugins.get(resource)
        if inst is None or self._stop.is_set():
            return
        threading.Thread(
            target=self.register, args=(inst,), daemon=True,
            name=f"reregister-{resource}",
        ).start()

    # ---- kubelet.sock watch ----

    def _socket_ident(self) -> Optional[tuple]:
        try:
            st = os.stat(self.kubelet_socket)
            # inode numbers get reused on tmpfs/overlay; ctime_ns
            # disambiguates a re-created socket with a recycled inode
            return (st.st_ino, st.st_dev, st.st_ctime_ns)
        except OSError:
            return None

    def _watch_loop(self, last: Optional[tuple]) -> None:
        while not self._stop.wait(self.watch_interval):
            cur = self._socket_ident()
            if cur is not None and cur != last:
                log.info("kubelet.sock (re)created; re-registering all plugins")
                for inst in list(self.plugins.values()):
                    # the restarted kubelet will reopen ListAndWatch; make
                    # sure it gets a fresh device/health snapshot even when
                    # no pulse ticker runs — both server implementations
                    try:
                        if inst.native:
                            inst.server.heartbeat()
                        else:
                            inst.plugin.heartbeat()
                    except Exception:
                        log.exception("state refresh failed")
                    self.register(inst)
            last = cur

    # ---- lifecycle ----

    def run(self, resources: List[str]) -> None:
        os.makedirs(self.device_plugin_path, exist_ok=True)
        # sample the socket before the first registration attempt: a kubelet
        # that comes up while registration is failing, or right after run()
        # returns, must look (re)created to the watch, not like the state it
        # started from (registering twice is harmless)
        seen = self._socket_ident()
        for res in resources:
            self.start_resource(res)
        self._watch_thread = threading.Thread(
            target=self._watch_loop, args=(seen,),
            daemon=True, name="kubelet-sock-watch",
        )
        self._watch_thread.start()

    def heartbeat_all(self) -> None:
        # snapshot: the ticker thread may race a start_resource dict insert
        for inst in list(self.plugins.values()):
            if inst.native:
                inst.server.heartbeat()  # recompute + push to all streams
            else:
                inst.plugin.heartbeat()

    def stop(self) -> None:
        self._stop.set()
        if self._watch_thread is not None:
            self._watch_thread.join(timeout=2)
        for inst in self.plugins.values():
            inst.plugin.stop()
            if inst.server is not None:
                inst.server.stop(grace=1).wait()
            if os.path.exists(inst.socket_path):
                try:
                    os.unlink(inst.socket_path)
                except OSError:
                    pass
        self.plugins.clear()
