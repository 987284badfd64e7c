import atexit
import os
import shutil
import tempfile

import pytest
import torch

# keep test-generated profiler artifacts out of the committed profiles/:
# a directory private to this run (a fixed shared name under the temp dir
# breaks as soon as another user has created it); child processes inherit
# the variable and reuse it
if "DDLB_PROFILE_DIR" not in os.environ:
    os.environ["DDLB_PROFILE_DIR"] = tempfile.mkdtemp(
        prefix="ddlb_test_profiles_")
    atexit.register(shutil.rmtree, os.environ["DDLB_PROFILE_DIR"],
                    ignore_errors=True)


def pytest_configure(config):
    config.addinivalue_line(
        "markers", "gpu: test requires a HIP GPU (run on the MI355X box)")


def pytest_collection_modifyitems(config, items):
    if torch.cuda.is_available():
        return
    skip = pytest.mark.skip(reason="no HIP device in this container")
    for item in items:
        if "gpu" in item.keywords:
            item.add_marker(skip)


@pytest.fixture
def free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port
