# Item-size knobs against the default: bench lines of config 2 and per-rank shares at N = 8, then a
# tiny frame's fixed cost. Results go to $OUT/sched (OUT defaults to bench_out).
set -o pipefail
OUT=${OUT:-bench_out}
S=$OUT/sched
mkdir -p $S
ms() { python -c "import json;j=json.load(open('$S/$1.json'));print(j['ms_per_step'])"; }
timeout -k 10 300 python bench.py --steps 3 --warmup 1 > $S/c2_default.json 2>/dev/null && echo "default $(ms c2_default)" &&
CRT_ITEM_CHUNKS=3 CRT_TAIL_CHUNKS=81 timeout -k 10 300 python bench.py --steps 3 --warmup 1 > $S/c2_k3t81.json 2>/dev/null && echo "K3 tail81 $(ms c2_k3t81)" &&
CRT_ITEM_CHUNKS=1 timeout -k 10 300 python bench.py --steps 3 --warmup 1 > $S/c2_k1.json 2>/dev/null && echo "K1 $(ms c2_k1)" &&
timeout -k 10 300 python -u tools/tile_timing.py --config 2 --ns 8 --all > $S/n8_default.txt 2>&1 && tail -1 $S/n8_default.txt &&
CRT_ITEM_CHUNKS=7 CRT_TAIL_CHUNKS=13 timeout -k 10 300 python -u tools/tile_timing.py --config 2 --ns 8 --all > $S/n8_k7t13.txt 2>&1 && tail -1 $S/n8_k7t13.txt &&
CRT_ITEM_CHUNKS=7 CRT_TAIL_CHUNKS=40 timeout -k 10 300 python -u tools/tile_timing.py --config 2 --ns 8 --all > $S/n8_k7t40.txt 2>&1 && tail -1 $S/n8_k7t40.txt &&
timeout -k 10 300 python bench.py --steps 5 --warmup 1 --width 64 --height 16 --spp 4 --full --no-cpu-baseline > $S/tiny.json 2>/dev/null && echo "tiny $(python -c "import json;j=json.load(open('$S/tiny.json'));print(j['ms_per_step'], j['roofline']['kernel_ms'])")"
