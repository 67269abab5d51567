"""Child process of tests/test_gpu_stream.py::test_capture_as_a_process_first_push: the first push this process makes is
the one it captures into a graph; the replays must equal an eager run made afterwards, with no allocation in between."""
import sys


def main():
    from tests.test_gpu_stream import Dev, capture_and_replay, same

    dev = Dev.of()
    replayed, eager, allocs, grown = capture_and_replay(dev, warm=False)
    ok = all(same(a, b) for a, b in zip(replayed, eager)) and allocs == 0 and grown == 0
    print("stream capture ok" if ok else f"stream capture differs: allocations {allocs}, bytes {grown}")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
