"""Writes tests/golden/cif_writers/: every case of tests/test_cif_writers_golden.py through the CIF writer it names.  Run
once with the writers as they were before ``write_cif`` and ``write_cif_symmetric`` shared a line builder; the test keeps
the shared builder to those bytes.  Plain text, a few hundred bytes a file.

usage: python tests/golden/make_golden_cif_writers.py"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))


def main():
    from cartnet_amd import predict
    from test_cif_writers_golden import DIR, cases
    os.makedirs(DIR, exist_ok=True)
    for name, (writer, entry) in cases().items():
        getattr(predict, writer)(os.path.join(DIR, name), entry)
        print(name)


if __name__ == "__main__":
    main()
