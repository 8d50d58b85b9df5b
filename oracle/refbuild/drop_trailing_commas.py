"""TEST INFRASTRUCTURE ONLY: a filter between the preprocessor and the compiler.

The reference's sim.cpp ends three template argument lists with a comma
("AgentStats,\n >>"), which the front end it was written for accepts and which
ISO C++, g++ and clang++ reject -- no header can change that.  This filter reads
preprocessed C++ on stdin and, only inside the lines that come from the file
named on the command line, drops a comma that directly precedes a closing '>'.
Such a comma has no other meaning a compiler could give it.  Nothing else is
touched and nothing is written anywhere but stdout.  The second argument is the
number of such commas the recipe expects (3: sim.cpp:1099, :1144, :1159); with
any other count the filter fails and writes nothing, so that a reference that has
changed is looked at and not rewritten somewhere else.
"""
import re
import sys


def main():
    target, expected = sys.argv[1], int(sys.argv[2])
    marker = re.compile(r'^# (\d+) "((?:[^"\\]|\\.)*)"')
    inside = False
    run, out, dropped = [], [], 0

    def flush():
        nonlocal dropped
        if run:
            text, k = re.subn(r",(\s*>)", r"\1", "".join(run))
            dropped += k
            out.append(text)
            run.clear()

    for line in sys.stdin:
        m = marker.match(line)
        if m:
            flush()
            inside = m.group(2) == target
            out.append(line)
        elif inside:
            run.append(line)
        else:
            out.append(line)
    flush()
    if dropped != expected:
        sys.stderr.write(f"drop_trailing_commas: {dropped} trailing commas in {target}, {expected} expected: "
                         "nothing written\n")
        sys.exit(1)
    sys.stdout.write("".join(out))
    sys.stderr.write(f"drop_trailing_commas: {dropped} dropped in {target}\n")


if __name__ == "__main__":
    main()
