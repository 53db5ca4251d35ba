"""The one runner of the graph-capture tools under tests/tools -- TEST INFRASTRUCTURE, not a test file.  A tool runs in a child
process (stream capture is process-wide state; a capture that goes wrong takes the process with it, not the test session) under a
time limit of its own with a grace period, once: a child that fails or is killed at its limit is a failure and is never started
again."""
import os
import subprocess
import sys

TOOLS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools")


def run_graph_tool(name, *args, limit=150):
    """tests/tools/<name> with args: it must exit 0 and print GRAPH_OK.  The assertion message carries the exit status (124: the
    limit) and the ends of both streams, the tool's last `stage:` line among them."""
    tool = os.path.join(TOOLS, name)   # (an absolute name stands as it is: the runner's own tests pass scripts of theirs)
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, tool, *args], capture_output=True, text=True,
                       timeout=limit + 20)
    assert r.returncode == 0 and "GRAPH_OK" in r.stdout, f"exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
