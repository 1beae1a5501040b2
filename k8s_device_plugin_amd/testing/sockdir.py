"""Where test and benchmark harnesses may bind unix sockets.

sockaddr_un.sun_path holds 107 bytes.  The harnesses bind names such as
<dir>/device-plugins/kubelet.sock below a fresh temporary directory, so the
directory they start from must leave room for that.
"""

from __future__ import annotations

import os
import tempfile

SUN_PATH_MAX = 107
# longest name bound below the root: a mkdtemp directory, a per-test
# directory, "device-plugins/" and a socket name such as
# "amd.com_cpx_nps2" -- about 70 bytes
ROOM_BELOW_ROOT = 75


def short_tmp_root() -> str:
    """The usual temporary directory if sockets fit below it, else the
    first writable standard one that is short enough."""
    usual = tempfile.gettempdir()
    for cand in (usual, "/tmp", "/var/tmp", "/dev/shm"):
        if (len(cand) + ROOM_BELOW_ROOT <= SUN_PATH_MAX
                and os.path.isdir(cand) and os.access(cand, os.W_OK)):
            return cand
    return usual
