"""The modem sender objects as a C compiler sees them: tests/c_callers/modem_tx_objects.c -- a payload from a v29_tx object
into a v29_rx object, by name -- is compiled `gcc -std=c99 -pedantic -Wall -Wextra -Werror` and as C++ against include/ alone
(test_c_callers.py's build), and runs on the GPU."""
import pytest

from test_c_callers import build, run


def test_modem_tx_objects_caller_compiles_and_links(built, tmp_path):
    build("modem_tx_objects", str(tmp_path))


@pytest.mark.gpu
def test_modem_tx_objects_caller_runs(built, tmp_path):
    out = run([build("modem_tx_objects", str(tmp_path))])
    assert "modem_tx_objects: ok" in out, out
