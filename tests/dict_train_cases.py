"""Sample records for the dictionary trainer's tests: the seeded log-line generator, and the crafted cases the
host walk (tests/test_dict_train_walk.py) and the device (tests/test_gpu_dict_train.py) are held against
tests/dict_train_model.py with.  A case is (name, buf, offs, lens, dict_size, k)."""
import random

import dict_train_model as model

PATHS = ["/api/v1/users", "/api/v1/orders", "/api/v1/orders/items", "/static/app.js", "/static/site.css", "/healthz", "/api/v2/search",
         "/login", "/logout", "/api/v1/cart"]
AGENTS = ["Mozilla/5.0 (X11; Linux x86_64) Chrome/126.0 Safari/537.36",
          "Mozilla/5.0 (Macintosh; Intel Mac OS X 14_5) Version/17.5 Safari/605.1.15",
          "curl/8.5.0", "python-requests/2.32.3"]
METHODS = ["GET", "GET", "GET", "POST", "PUT", "DELETE"]


def log_lines(count, seed):
    """JSON-like access-log lines, about 290 bytes each.  Few templates — a request line, an upstream error, an auth event and
    a cache event, the request line the most frequent — so that a few KiB of raw records do not hold all of them and 32 KiB do;
    inside a template the fields vary."""
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        ts = "2026-03-%02dT%02d:%02d:%02d.%03dZ" % (rng.randint(1, 28), rng.randint(0, 23), rng.randint(0, 59), rng.randint(0, 59),
                                                     rng.randint(0, 999))
        addr = "10.%d.%d.%d" % (rng.randint(0, 255), rng.randint(0, 255), rng.randint(1, 254))
        rid = "%024x" % rng.getrandbits(96)
        kind = rng.random()
        if kind < 0.55:
            line = ('{"timestamp":"%s","level":"info","remote_addr":"%s","method":"%s","path":"%s","status":%d,"bytes_sent":%d,'
                    '"request_time":%.3f,"request_id":"%s","upstream":"backend-%02d.internal:8080","user_agent":"%s"}\n'
                    % (ts, addr, rng.choice(METHODS), rng.choice(PATHS), rng.choice([200, 200, 200, 201, 204, 301, 304, 400, 404, 500]),
                       rng.randint(0, 250000), rng.random() * 2, rid, rng.randint(1, 12), rng.choice(AGENTS)))
        elif kind < 0.70:
            line = ('{"timestamp":"%s","level":"error","request_id":"%s","upstream":"backend-%02d.internal:8080","event":"upstream_error",'
                    '"message":"upstream timed out (110: Connection timed out) while reading response header from upstream",'
                    '"retries":%d,"path":"%s","remote_addr":"%s"}\n'
                    % (ts, rid, rng.randint(1, 12), rng.randint(0, 3), rng.choice(PATHS), addr))
        elif kind < 0.85:
            line = ('{"timestamp":"%s","level":"notice","event":"auth","outcome":"%s","user_id":%d,"session":"%016x","remote_addr":"%s",'
                    '"mechanism":"oauth2-bearer","scopes":["profile","orders:read","orders:write"],"token_age_seconds":%d,'
                    '"request_id":"%s"}\n'
                    % (ts, rng.choice(["accepted", "accepted", "refreshed", "rejected"]), rng.randint(1000, 99999), rng.getrandbits(64), addr,
                       rng.randint(0, 86400), rid))
        else:
            line = ('{"timestamp":"%s","level":"debug","event":"cache","result":"%s","key":"tenant:%d:catalog:item:%d","ttl_seconds":%d,'
                    '"node":"cache-%02d.internal:6379","size_bytes":%d,"request_id":"%s","path":"%s","latency_us":%d}\n'
                    % (ts, rng.choice(["hit", "hit", "miss", "stale"]), rng.randint(1, 40), rng.randint(1, 500000), rng.randint(0, 3600),
                       rng.randint(1, 6), rng.randint(100, 90000), rid, rng.choice(PATHS), rng.randint(50, 20000)))
        out.append(line.encode())
    return out


def flat(records, gaps=None, junk=0xFF):
    """records (bytes) laid out one after the other → (buf, offs, lens); gaps[i] junk bytes in front of record i"""
    buf, offs = bytearray(), []
    for i, r in enumerate(records):
        if gaps:
            buf += bytes([junk]) * gaps[i]
        offs.append(len(buf))
        buf += r
    return bytes(buf), offs, [len(r) for r in records]


def _noise(rng, n):
    return bytes(rng.getrandbits(8) for _ in range(n))


def cases():
    rng = random.Random(20260301)
    out = []

    def add(name, records, size, k, gaps=None):
        buf, offs, lens = flat(records, gaps)
        out.append((name, buf, offs, lens, size, k))

    lines = log_lines(200, 11)
    add("shorter_than_a_dmer", [b"abcde"], 64, 16)
    add("exactly_k", [lines[0][:128]], 256, 128)
    add("k_minus_1", [lines[0][:127]], 256, 128)
    add("tiny_among_longer", [lines[0], b"1234567", lines[1], b"12345678", b"123456789", lines[2], b"", lines[3]] + lines[4:40], 1024, 64)
    add("n_below_epochs", [lines[0][:100], lines[1][:100], lines[2][:100]], 32768, 16)
    add("identical_records", [lines[5][:200]] * 64, 2048, 128)
    # two records of k bytes whose d-mers are all distinct: every counter they touch is 1, both candidates score k - 7
    a, b = _noise(rng, 128), _noise(rng, 128)
    add("tie_in_one_epoch", [a, b], 128, 128)
    add("tie_across_epochs", [a, b], 256, 128)
    add("size_no_multiple_of_k", lines, 1000, 128)
    add("smallest", lines[:50], 64, 16)
    add("k_is_dict_size_64", lines[:50], 64, 64)
    add("k_is_dict_size_256", lines[:50], 256, 256)
    # hot: 128 bytes whose halves are frequent, in records too short to hold a candidate; it appears whole only across the
    # seam of two records of k bytes, where no candidate may lie
    hot = _noise(rng, 128)
    add("seam", [_noise(rng, 64) + hot[:64], hot[64:] + _noise(rng, 64)] + [hot[:64], hot[64:]] * 40, 128, 128)
    more = log_lines(300, 12)
    add("gaps", [r if i % 17 else b"" for i, r in enumerate(more)], 4096, 128, gaps=[rng.randint(0, 13) for _ in more])
    return out


def big_cases():
    """the generator's records at scale: 4096 records at two sizes; 8192 records in ONE epoch — more chunks than the epoch step
    has workgroups, more positions than the count kernel's grid covers in one pass"""
    recs = log_lines(8192, 13)
    buf, offs, lens = flat(recs[:4096])
    out = [("gen4096_size2048", buf, offs, lens, 2048, 128), ("gen4096_size32768", buf, offs, lens, 32768, 128)]
    buf, offs, lens = flat(recs)
    out.append(("gen8192_one_epoch", buf, offs, lens, 128, 128))
    return out


def expect(case):
    _name, buf, offs, lens, size, k = case
    return model.train_flat(buf, offs, lens, size, k)
