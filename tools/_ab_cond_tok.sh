# same-box interleaved A/B of the token form of the stack launch (profiles/r07_cond_tok_ab.log):
#   tools/_ab_cond_tok.sh <library built with -DBSG_CQ_TOK_AUX=3> <checkout of the parent commit, built>
# BSG_COND_TOK=0 / default / the cache-policy variant (BSG_LIB) / the parent's tree and library; three repetitions of bench.py --steps 5.
# The parent runs from its own tree: its binding refuses this tree's ABI.  Stops at the first run that fails.
R=$PWD
one() {  # label dir env...
  label=$1; dir=$2; shift 2
  line=$(cd $dir && env "$@" timeout -k 10 200 python bench.py --no-secondary --cpu-steps 0 --steps ${AB_STEPS:-5} 2>/dev/null | tail -1) || { echo "$label failed"; exit 1; }
  echo "$label $line"
}
for rep in 1 2 3; do
  one off$rep $R BSG_COND_TOK=0
  one on$rep $R BSG_COND_TOK=1
  [ -n "$1" ] && one aux3_$rep $R BSG_LIB=$1
  [ -n "$2" ] && one parent$rep $2 BSG_COND_TOK=1
done
